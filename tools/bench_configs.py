#!/usr/bin/env python3
"""Secondary workloads of BASELINE.json (configs[2], configs[3]) and the other byte kernels, kernel time by HIP events.
Not the driver's bench line (bench.py is); the numbers go to DESIGN.md §6.
  configs[2]: WeightedMovingVarianceBGS + AdaptiveBackgroundLearning, 3840x2160 (HBM-bound stress)
  configs[3]: LBSP descriptor path, 1920x1080
  --only kde: KDE (package_bgs/ae) young / aged model, static and ~10 % foreground scenes, 8 x 1080p
  --only dp2: DPPratiMediodBGS (sampled / other frames) and DPTextureBGS, 8 x 1080p
  --only lb: the five package_bgs/lb models (double-precision planes), static and ~10 % foreground scenes, SOMs inside and past their
             calibration phase, the Gaussian pair with one and two pixels per lane, 8 x 1080p  (lb_<class>: one class, short legs);
             then clip calls of T = 4 and 8 frames, fused and frame by frame alternating  (lb_clip: these legs alone)
  --only vumeter: VuMeter (package_bgs/av), dense and live-bin kernels (BGS_VU_SPARSE 0 / 1 / 2), filter on and off, on S_surv and on
             fresh uniform noise (every bin live: the live-bin kernels' worst case), 8 x 1080p
  --only fuzzy: FuzzySugenoIntegral and FuzzyChoquetIntegral (package_bgs/tb), ms per learning step and per detecting step on S_surv,
             8 x 1080p  (fuzzy_choquet / fuzzy_sugeno: one class, short legs, no calibration: for kernel-trace passes)
  --only t2f: T2FGMM_UM and T2FGMM_UV (package_bgs/tb) beside DPGrimsonGMM timed in the same process, reference defaults (K = 3), on
             S_surv, 8 x 1080p: ms per step and ms per frame at clip T = 8
  --only eigen: DPEigenbackgroundBGS (package_bgs/dp) beside DPGrimsonGMM timed in the same process, reference defaults (H = 20, M = 10),
             on S_surv, 8 x 1080p and 1 x 1080p: ms per detecting step, the one-off model build at frame H, this box's copy rate
  --only imbs: IndependentMultimodalBGS (package_bgs/db) at the wrapper's defaults (numSamples 30) on S_surv, 8 x 1080p: the detect-only
             step, the sampling step and the build step apart, what the launches cost on empty planes, the numpy restatement beside
  --only multilayer: MultiLayerBGS (package_bgs/jmo) at the wrapper's defaults on S_surv, 8 x 1080p: ms per step, the model kernel and
             the smoothing kernel apart, bytes per pixel of state, this box's copy rate
  --only canny: bgs_canny_device on 160 x 120 images (the reduced frame of package_bgs/sjn), batches of 1 to 256: a block scene, uniform
             noise, and a serpentine whose hysteresis has to walk one chain of 2357 pixels; the numpy restatement beside
  --only multicue: the model stage, the box stage and the whole step of SJN_MultiCueBGS (bgs_multicue) at the reference's defaults, 8 and 32 streams of 1080p frames reduced
             to 160 x 120: us per train, landmark and update call, bytes of state per reduced pixel, the live bytes a call touches
             over this box's copy rate; the 32-stream step as two ranges on two HIP streams beside the one call; the host path of one
             1080p camera (upload + step + download)
  --only lbpmrf_mask: bgs_lbpmrf_mask_device (the grid min-cut and the mask of LbpMrf) on 1, 8 and 32 rate maps of a 1080p frame
             (1076 x 958 nodes): blob-like maps, uniform noise and an all-neutral map; us per call, the relaxation launches a call used,
             and the max-flow / min-cut duality of every map as the leg's own check
usage: bench_configs.py [--streams S] [--swizzle 0|1]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools import synth
from tracking_amd import Engine, capi
from tracking_amd.engine import lbsp_describe_device


def cpu_rate(algo, frames_np, warm=3, params=None):
    """The oracle (CPU restatement, 1 thread; rows split over the box's quota for the MOG loops) on a few frames of the same size."""
    from oracle import pyoracle
    import os
    threads = 1
    if algo in (capi.MOG2, capi.MOG1):
        try:
            q, per = open("/sys/fs/cgroup/cpu.max").read().split()
            threads = min(len(os.sched_getaffinity(0)), int(int(q) / int(per))) if q != "max" else 16
        except Exception:
            threads = 16
    o = pyoracle.Oracle(algo, params=params, threads=threads)
    for f in frames_np[:warm]:
        o.process(f, want_bg=False)
    t0 = time.perf_counter()
    n = 0
    for f in frames_np[warm:]:
        o.process(f, want_bg=False)
        n += 1
    dt = time.perf_counter() - t0
    return n * frames_np.shape[1] * frames_np.shape[2] / dt / 1e6, threads


# Bytes MOVED per pixel by the kernels whose traffic depends on the data (the mixture models read only the modes a pixel has and write
# only what changed; GMG walks a per-pixel list): measured with rocprofv3 --pmc (FETCH_SIZE x 2 + WRITE_SIZE) on these very legs -
# profiles/r03_mog1_pmc.txt, profiles/r03_dp_pmc.txt, DESIGN.md 9 (GMG).  Round 3 priced these legs at the DENSE sorted-array figure of
# SURVEY.md 8(a) and printed "fractions" of 150-240 %: not fractions of anything.  A leg without a measurement prints no fraction.
MOVED_BPP = {(capi.MOG1, "surv"): 97, (capi.MOG1, "sat"): 171, (capi.DP_ZIVKOVIC_AGMM, "sat"): 98, (capi.DP_ZIVKOVIC_AGMM, "surv"): 42,
             (capi.DP_GRIMSON_GMM, "sat"): 122, (capi.GMG, "surv"): 76}
DATA_DEPENDENT = (capi.MOG1, capi.MOG2, capi.DP_ZIVKOVIC_AGMM, capi.DP_GRIMSON_GMM, capi.GMG)


def run(algo, name, rows, cols, S, bpp, steps=60, borrow=True, want_bg=False, cpu_frames=6, cpu_warm=3, params=None, kind="surv"):
    dev = torch.device("cuda", 0)
    T = 10 if kind == "sat" else 8  # S_sat repeats every 5 frames: the pool must wrap at a multiple of 5
    pool = torch.empty((T, S, rows, cols, 3), dtype=torch.uint8, device=dev)
    for s in range(S):
        pool[:, s] = (synth.s_surv if kind == "surv" else synth.s_sat)(T, rows, cols, seed=4321 + s, device=dev)
    e = Engine(algo, n_streams=S, params=params)
    e.set_geometry(rows, cols, 3)
    if borrow:
        e.set_option(capi.OPT_BORROW_FRAMES, 1)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    bg = torch.empty((S, rows, cols, 3), dtype=torch.uint8, device=dev) if want_bg else None
    # mixture models on S_sat need ~100 frames before the weights have equalised and every frame re-orders the modes (steady-state
    # traffic; a younger model writes less and flatters the figure - round-2 verdict); everything else is warm after 10
    mixture = algo in (capi.MOG2, capi.MOG1, capi.DP_ZIVKOVIC_AGMM, capi.DP_GRIMSON_GMM)
    nwarm = 140 if (mixture and kind == "sat") else (40 if mixture else 10)
    for t in range(nwarm):
        e.process_batch_device(pool[t % T], fg, bg, None)
    torch.cuda.synchronize()
    e.enable_kernel_timing(True)
    t0 = time.perf_counter()
    for t in range(steps):
        e.process_batch_device(pool[(nwarm + t) % T], fg, bg, None)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms, n, kname = e.kernel_timing()
    px = S * rows * cols
    cpu = ""
    if cpu_frames:
        sample = pool[:cpu_frames, 0].cpu().numpy() if T >= cpu_frames else torch.cat([pool[:, 0]] * (cpu_frames // T + 1))[:cpu_frames].cpu().numpy()
        rate, th = cpu_rate(algo, sample, warm=cpu_warm, params=params)
        cpu = " | CPU oracle %.1f Mpix/s (%d thread%s)" % (rate, th, "s" if th > 1 else "")
    if algo in DATA_DEPENDENT:
        moved = MOVED_BPP.get((algo, kind))
        rate = ("%7.1f GB/s moved (%d B/px by PMC on this leg) = %.1f%% of 8 TB/s" % (moved * px / ms / 1e6, moved, moved * px / ms / 1e6 / 80.0)) if moved else "traffic data-dependent, not measured on this leg: no fraction"
        rate += " [dense sorted-array figure of SURVEY.md 8(a): %d B/px - not moved]" % bpp
    else:
        rate = "%7.1f GB/s algorithmic (%d B/px) = %.1f%% of 8 TB/s" % (bpp * px / ms / 1e6, bpp, bpp * px / ms / 1e6 / 80.0)
    print("%-34s %dx%d x%d streams: kernel %-18s %.4f ms  -> %8.1f Mpix/s  %s | wall %.1f Mpix/s%s"
          % (name, cols, rows, S, kname, ms, px / ms / 1e3, rate, px * steps / wall / 1e6, cpu))
    e.close()


def run_subsense(S, steps=30, kind="surv", algo=None, label="SuBSENSEBGS", warm=6, groups=1):
    """BASELINE configs[3]: SuBSENSE at 1920x1080 (per-frame wall time: ~20 launches incl. the flood-fill host loop)."""
    dev = torch.device("cuda", 0)
    rows, cols, T = 1080, 1920, 8
    pool = torch.empty((T, S, rows, cols, 3), dtype=torch.uint8, device=dev)
    for s in range(S):
        pool[:, s] = (synth.s_surv if kind == "surv" else synth.s_smooth)(T, rows, cols, seed=4321 + s, device=dev)
    e = Engine(capi.SUBSENSE if algo is None else algo, n_streams=S)
    e.set_geometry(rows, cols, 3)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    # groups > 1: the batch as `groups` stream ranges, each on its own HIP stream (bgs_process_range_device): one range's memory-bound
    # tail (sample writes, post-processing) then runs beside another range's VALU-bound phase A
    hs = [torch.cuda.Stream() for _ in range(groups)] if groups > 1 else None
    per = S // groups

    def step(t):
        if groups == 1:
            e.process_batch_device(pool[t % T], fg, None, None)
        else:
            for g in range(groups):
                e.process_batch_device(pool[t % T, g * per:(g + 1) * per], fg[g * per:(g + 1) * per], None, None, hip_stream=hs[g].cuda_stream, first=g * per, count=per)
    for t in range(warm):
        step(t)
    torch.cuda.synchronize()
    e.enable_kernel_timing(True)
    t0 = time.perf_counter()
    for t in range(steps):
        step(warm + t)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    ms, n, kname = e.kernel_timing()
    px = S * rows * cols
    print("%-34s %dx%d x%d streams: %.3f ms/frame-step wall -> %8.1f Mpix/s (%.1f 1080p frames/s); %s %.3f ms; fg ratio %.3f"
          % ("%s (%s input%s%s)" % (label, kind, "" if warm == 6 else ", model aged %d frames" % warm, "" if groups == 1 else ", %d ranges on %d HIP streams" % (groups, groups)), cols, rows, S, wall * 1e3, px / wall / 1e6, S / wall, kname, ms, float((fg != 0).float().mean())))
    e.close()


def run_lbsp():
    # LBSP descriptors, 1080p
    img = synth.s_surv(1, 1080, 1920, seed=9, device="cuda")[0]
    from oracle import pyoracle
    lut = pyoracle.lbsp_lut(0.333, 0, 3)
    out = torch.empty((1080, 1920, 3), dtype=torch.int16, device="cuda")
    for _ in range(5):
        lbsp_describe_device(img, lut, out=out)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(50):
        lbsp_describe_device(img, lut, out=out)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / 50
    px = 1080 * 1920
    print("%-34s 1920x1080 x1: %.4f ms -> %8.1f Mpix/s  %7.1f GB/s algorithmic (9 B/px)" % ("LBSP descriptors (lbsp_kernel)", ms, px / ms / 1e3, 9 * px / ms / 1e6))
    from tracking_amd.engine import lbsp_describe_batch_device
    imgs = synth.s_surv(16, 1080, 1920, seed=9, device="cuda")
    for _ in range(3):
        lbsp_describe_batch_device(imgs, lut)
    torch.cuda.synchronize()
    a.record()
    for _ in range(20):
        lbsp_describe_batch_device(imgs, lut)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / 20
    px = 16 * 1080 * 1920
    print("%-34s 1920x1080 x16 (one launch): %.4f ms -> %8.1f Mpix/s  %7.1f GB/s algorithmic (9 B/px, incl. the output allocation)" % ("LBSP descriptors (lbsp_kernel)", ms, px / ms / 1e3, 9 * px / ms / 1e6))



def run_pipeline(S=8, steps=30):
    """Frames in HBM -> SuBSENSE masks -> blob rectangles, all on the device; only the boxes and offsets cross PCIe."""
    from tracking_amd.engine import mask_components_batch_device
    dev = torch.device("cuda", 0)
    rows, cols, T = 1080, 1920, 8
    pool = torch.empty((T, S, rows, cols, 3), dtype=torch.uint8, device=dev)
    for s in range(S):
        pool[:, s] = synth.s_surv(T, rows, cols, seed=4321 + s, device=dev)
    e = Engine(capi.SUBSENSE, n_streams=S)
    e.set_geometry(rows, cols, 3)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    for t in range(6):
        e.process_batch_device(pool[t % T], fg, None, None)
    torch.cuda.synchronize()
    nbox = nbytes = 0
    t0 = time.perf_counter()
    for t in range(steps):
        e.process_batch_device(pool[(6 + t) % T], fg, None, None)
        _, boxes, off = mask_components_batch_device(fg, 8, max_boxes=65536)
        host = boxes.cpu()
        nbox += host.shape[0]
        nbytes += host.numel() * 4 + off.numel() * 4
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    print("pipeline SuBSENSE -> components  1920x1080 x%d streams: %.3f ms per step = %.1f 1080p frames/s end to end; %.1f boxes and %.0f bytes D2H per step "
          "(full masks would be %d bytes)" % (S, wall * 1e3, S / wall, nbox / steps, nbytes / steps, S * rows * cols))
    # The same, as a streaming consumer would drive it: nothing waits for step t before step t+1 is enqueued - two sets of output
    # buffers, the boxes of step t go to pinned memory asynchronously and are read when the event behind that copy has fired, one step late.
    import ctypes as C
    max_boxes = 65536
    lib = capi.lib()
    wsz = lib.bgs_mask_components_batch_workspace(S, rows, cols)
    fgs = [torch.empty((S, rows, cols), dtype=torch.uint8, device=dev) for _ in range(2)]
    boxes = [torch.zeros((max_boxes, 6), dtype=torch.int32, device=dev) for _ in range(2)]
    offs = [torch.zeros(S + 1, dtype=torch.int32, device=dev) for _ in range(2)]
    work = [torch.empty(wsz, dtype=torch.uint8, device=dev) for _ in range(2)]
    hbox = [torch.zeros((4096, 6), dtype=torch.int32).pin_memory() for _ in range(2)]
    hoff = [torch.zeros(S + 1, dtype=torch.int32).pin_memory() for _ in range(2)]
    ev = [torch.cuda.Event() for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    nbox = 0
    e.close()
    e = Engine(capi.SUBSENSE, n_streams=S)  # a fresh model, the same 6 warm-up frames: comparable with the figure above
    e.set_geometry(rows, cols, 3)
    for t in range(6):
        e.process_batch_device(pool[t % T], fg, None, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps + 1):
        i = t & 1
        if t < steps:
            e.process_batch_device(pool[(6 + t) % T], fgs[i], None, None)
            capi.check(lib.bgs_mask_components_batch_device(0, C.c_void_p(fgs[i].data_ptr()), S, rows, cols, 8, None, C.c_void_p(boxes[i].data_ptr()), max_boxes,
                                                            C.c_void_p(offs[i].data_ptr()), C.c_void_p(work[i].data_ptr()), C.c_void_p(stream)))
            hbox[i].copy_(boxes[i][:4096], non_blocking=True)
            hoff[i].copy_(offs[i], non_blocking=True)
            ev[i].record()
        if t >= 1:
            j = (t - 1) & 1
            ev[j].synchronize()
            nbox += int(hoff[j][-1])
    wall2 = (time.perf_counter() - t0) / steps
    print("pipeline, consumer one step behind   1920x1080 x%d streams: %.3f ms per step = %.1f 1080p frames/s end to end; %.1f boxes per step"
          % (S, wall2 * 1e3, S / wall2, nbox / steps))
    e.close()


def run_dp():
    """N4: the package_bgs/dp models at 1080p x 16 streams (state r/w + frame + mask bytes per pixel)."""
    run(capi.DP_ZIVKOVIC_AGMM, "DPZivkovicAGMMBGS (K=3, S_sat)", 1080, 1920, 16, 126, borrow=False, kind="sat", cpu_frames=0)
    run(capi.DP_GRIMSON_GMM, "DPGrimsonGMMBGS (K=3, S_sat)", 1080, 1920, 16, 150, borrow=False, kind="sat", cpu_frames=0)
    run(capi.DP_ZIVKOVIC_AGMM, "DPZivkovicAGMMBGS (K=3, S_surv)", 1080, 1920, 16, 126, borrow=False)
    run(capi.DP_GRIMSON_GMM, "DPGrimsonGMMBGS (K=3, S_surv)", 1080, 1920, 16, 150, borrow=False)
    run(capi.DP_WREN_GA, "DPWrenGABGS", 1080, 1920, 16, 36, borrow=False)
    run(capi.DP_MEAN, "DPMeanBGS", 1080, 1920, 16, 28, borrow=False)
    run(capi.DP_ADAPTIVE_MEDIAN, "DPAdaptiveMedianBGS", 1080, 1920, 16, 7, borrow=False)  # 3 frame + 3 median + 1 mask (+3/7 write-back); state is MALL-resident


def run_cc():
    """N1: connected components of a 1080p foreground-like mask (blobs + salt noise) and of a worst case (random 45 %)."""
    import numpy as np
    from tracking_amd.engine import mask_components_device
    rng = np.random.default_rng(1)
    blobs = np.zeros((1080, 1920), np.uint8)
    for _ in range(60):
        y, x = rng.integers(0, 1000), rng.integers(0, 1800)
        blobs[y:y + rng.integers(5, 80), x:x + rng.integers(5, 120)] = 255
    blobs[rng.random(blobs.shape) < 0.001] = 255
    for name, m in (("blobs+noise", blobs), ("random 45%", np.where(rng.random((1080, 1920)) < 0.45, 255, 0).astype(np.uint8)), ("full", np.full((1080, 1920), 255, np.uint8))):
        d = torch.from_numpy(m).cuda()
        for _ in range(3):
            labels, boxes, n = mask_components_device(d, 8, max_boxes=65536)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            labels, boxes, n = mask_components_device(d, 8, max_boxes=65536)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / 20
        print("connected components 1920x1080 %-12s: %d components, %.3f ms per mask (incl. count read-back) -> %.1f Mpix/s" % (name, n, ms, 1080 * 1920 / ms / 1e3))


def run_canny(rows=120, cols=160, reps=50):
    """bgs_canny_device: one workgroup per image, so a call costs what its slowest image costs until the batch outgrows the CUs."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import canny_numpy as cn
    from tracking_amd.engine import canny_device
    rng = np.random.default_rng(3)
    coarse = rng.integers(0, 256, (rows // 8, cols // 8), dtype=np.uint8)
    snake = np.zeros((rows, cols), np.uint8)
    for j in range((rows - 8) // 8 + 1):
        snake[8 * j + 2:8 * j + 6, 2:cols - 2] = 35
        if j + 1 < (rows - 8) // 8 + 1:
            c = cols - 6 if j % 2 == 0 else 2
            snake[8 * j + 6:8 * j + 10, c:c + 4] = 35
    snake[2:6, 2:6] = 255
    scenes = (("8 x 8 blocks", np.repeat(np.repeat(coarse, 8, 0), 8, 1), 100, 150), ("uniform noise", rng.integers(0, 256, (rows, cols), dtype=np.uint8), 100, 150),
              ("serpentine", snake, 100, 250))
    for name, img, low, high in scenes:
        t0 = time.perf_counter()
        want = cn.canny(img, low, high)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        for images in (1, 8, 64, 256):
            d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(img, (images, rows, cols)))).cuda()
            for _ in range(3):
                out = canny_device(d, low, high)
            torch.cuda.synchronize()
            assert np.array_equal(out[images - 1].cpu().numpy(), want)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                out = canny_device(d, low, high)
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) / reps * 1e3
            print("canny %dx%d %-14s %3d images: %8.1f us per call, %7.2f us per image, %d edge pixels  (numpy restatement %.1f ms per image)"
                  % (cols, rows, name, images, us, us / images, int((want == 255).sum()), cpu_ms))


def run_lbpmrf_mask(rows=1080, cols=1920, reps=5):
    """bgs_lbpmrf_mask_device: a fixed budget of step launches per call, of which the first `launches` work and the rest return at once.  The
    reference is not needed: the labels describe a cut, and a cut whose capacity equals the flow value is a minimum cut of a maximum flow."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import lbpmrf_numpy as ln
    import lbpmrf_scenes as sc
    from tracking_amd.engine import lbpmrf_mask_counters, lbpmrf_mask_device
    nh, nw = sc.nodes(rows, cols)
    makers = (("blobs", lambda k: sc.blobs(nh, nw, 1 + k)), ("uniform noise", lambda k: sc.uniform(nh, nw, 2 + k)), ("all neutral", lambda k: sc.neutral(nh, nw)))
    for name, make in makers:
        distinct = [make(k) for k in range(4)]
        for images in (1, 8, 32):
            rates = np.stack([distinct[k % 4] for k in range(images)])
            d = torch.from_numpy(rates).cuda()
            mask, labels, flow = lbpmrf_mask_device(d, rows, cols)
            torch.cuda.synchronize()
            stuck, launches = lbpmrf_mask_counters()
            assert stuck == 0, "the cut did not converge within its launches"
            labels_h, flow_h = labels.cpu().numpy(), flow.cpu().numpy()
            for k in range(min(images, 4)):
                cut = ln.duality(ln.sink_weights(rates[k]), labels_h[k])
                assert cut == int(flow_h[k]), ("duality", name, images, k, cut, int(flow_h[k]))
            for k in range(4, images):  # the repeats of the batch
                assert np.array_equal(labels_h[k], labels_h[k % 4]) and flow_h[k] == flow_h[k % 4]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                mask, labels, flow = lbpmrf_mask_device(d, rows, cols)
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) / reps * 1e3
            print("lbpmrf_mask %dx%d (%d x %d nodes) %-14s %2d maps: %10.1f us per call, %9.1f us per map, %3d relaxation launches used, SINK nodes of map 0 %d, "
                  "foreground pixels of map 0 %d, duality holds" % (cols, rows, nh, nw, name, images, us, us / images, launches, int(labels_h[0].sum()), int((mask[0] != 0).sum())))
    assert lbpmrf_mask_counters()[0] == 0


def run_multicue(rows=1080, cols=1920, reps=30):
    """bgs_multicue at the defaults (160 x 120 reduced pixels per stream whatever the frame size): a call is three preprocessing launches
    and one model launch over S x 19 200 pixels, so it is bound by launches, not by bytes, until S is large."""
    from tracking_amd.engine import MultiCueModel
    copy = capi.calibrate_copy(0, 2 << 30, 0)
    T, TC, CS, CC = capi.MULTICUE_TEXTURE_SLOTS, capi.MULTICUE_TEXTURE_CACHE_SLOTS, capi.MULTICUE_COLOR_SLOTS, capi.MULTICUE_COLOR_CACHE_SLOTS
    state = 6 * (T + TC) * 16 + 6 * 2 * 8 + (CS + CC) * 36 + 2 * 8 + 7 * 4 + 9 + 4 + 1
    print("multicue: %d bytes of state per reduced pixel (slots %d / %d / %d / %d); copy rate of this box %.0f GB/s" % (state, T, TC, CS, CC, copy))
    for S in (8, 32):
        g = torch.Generator(device="cuda").manual_seed(5)
        coarse = torch.randint(0, 256, (S, rows // 8, cols // 8, 3), generator=g, device="cuda", dtype=torch.int16)
        base = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2)
        pool = [(base + torch.randint(-2, 3, base.shape, generator=g, device="cuda", dtype=torch.int16)).clamp_(0, 255).to(torch.uint8) for _ in range(3)]
        moved = [f.clone() for f in pool]
        for f in moved:
            f[:, rows // 4:rows // 2, cols // 4:cols // 2] = 200  # a block the model has not seen
        p = capi.multicue_default_params()
        um = torch.ones((S, p.reduced_height, p.reduced_width), dtype=torch.uint8, device="cuda")
        um[:, p.reduced_height // 4:p.reduced_height // 2, p.reduced_width // 4:p.reduced_width // 2] = 0
        times = {"train": [], "landmark": [], "update": []}

        def timed(kind, call, *a, **kw):
            a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            out = call(*a, **kw)
            b0.record()
            times[kind].append((a0, b0))
            return out

        with MultiCueModel(p, n_streams=S) as m:
            for t in range(p.training_period + 1):
                timed("train", m.train, pool[t % 3])
            for t in range(reps + 3):
                timed("landmark", m.landmark, moved[t % 3])
                timed("update", m.update, um)
            torch.cuda.synchronize()
            assert m.state("overflow")[0] == 0
            live = sum(int(m.state(k)[..., 1].sum()) * b for k, b in (("tbook", 16), ("tcache", 16), ("cbook", 36), ("ccache", 36)))
        n = p.reduced_height * p.reduced_width
        for kind, ev in times.items():
            us = np.array([a0.elapsed_time(b0) * 1e3 for a0, b0 in ev[3:]])
            rw = {"train": 2, "landmark": 1, "update": 2}[kind]  # the live entries read (and written back) once
            gbs = (S * live * rw + S * n * 16) / (np.median(us) * 1e-6) / 1e9
            print("multicue %2d x %dx%d -> 160x120 %-8s: median %7.1f us per call (min %.1f, max %.1f, %d calls), %d launches; live state of stream 0 %d B/px -> at most about %.1f GB/s = %.3f of the copy rate (every live entry read and written once)%s"
                  % (S, cols, rows, kind, np.median(us), us.min(), us.max(), len(us), 1 if kind == "update" else 4, live // n, gbs, gbs / copy, " (launch-bound)" if gbs / copy < 0.1 else ""))

        # the box stage (three launches: per-pixel preparation, one labelling workgroup per stream, one workgroup per (stream, box) slot) on
        # the landmark map of the moved scene, on an empty map (the labelling chain alone: no box survives) and on a full one (one box with
        # the largest window); then the whole step (ten launches)
        def median_us(call, *a, n_calls=reps + 3):
            ev = []
            for _ in range(n_calls):
                a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a0.record()
                call(*a)
                b0.record()
                ev.append((a0, b0))
            torch.cuda.synchronize()
            us = np.array([a0.elapsed_time(b0) * 1e3 for a0, b0 in ev[3:]])
            return np.median(us), us.min(), us.max(), len(us)

        with MultiCueModel(p, n_streams=S) as m:
            for t in range(p.training_period + 1):
                m.process(pool[t % 3])
            lm, _ = m.landmark(moved[0], want_conf=False)
            m.update(um, ghost=True), m.update(um)
            for name, lmap in (("scene", lm), ("empty", torch.zeros_like(lm)), ("full", torch.full_like(lm, 255))):
                count = m.boxes(lmap, moved[0])[3]
                med, lo, hi, k = median_us(m.boxes, lmap, moved[0])
                print("multicue %2d x %dx%d -> 160x120 boxes/%-5s: median %7.1f us per call (min %.1f, max %.1f, %d calls), 3 launches; %d labels in stream 0"
                      % (S, cols, rows, name, med, lo, hi, k, int(count[0])))
            med, lo, hi, k = median_us(lambda: [m.process(moved[t % 3]) for t in range(3)], n_calls=reps // 3 + 3)
            assert m.state("overflow")[0] == 0 and m.state("box_overflow")[0] == 0
            print("multicue %2d x %dx%d -> 160x120 process     : median %7.1f us per call (min %.1f, max %.1f, %d triples of calls), 10 launches; %.2f us per stream"
                  % (S, cols, rows, med / 3, lo / 3, hi / 3, k, med / 3 / S))
            if S == 32:  # the same detecting step as two ranges of 16 streams on two HIP streams (bgs_multicue_process_range_device), beside the one call above
                side = [torch.cuda.Stream(), torch.cuda.Stream()]
                cur = torch.cuda.current_stream()

                def halves():
                    for t in range(3):
                        for h, s in enumerate(side):
                            s.wait_stream(cur)  # the timing event before this call is on the current stream
                            m.process(moved[t % 3][16 * h:16 * h + 16], first=16 * h, count=16, hip_stream=s.cuda_stream)
                        for s in side:
                            cur.wait_stream(s)

                med2, lo2, hi2, k2 = median_us(halves, n_calls=reps // 3 + 3)
                assert m.state("overflow")[0] == 0 and m.state("box_overflow")[0] == 0
                print("multicue 32 x %dx%d -> 160x120 process as [0,16) + [16,32) on two HIP streams: median %7.1f us per step (min %.1f, max %.1f, %d triples of steps), 2 x 10 launches; the one call: %.1f us"
                      % (cols, rows, med2 / 3, lo2 / 3, hi2 / 3, k2, med / 3))

    # the host path of one camera (bgs_multicue_process): a 1080p frame from pageable memory into page-locked staging, upload, the detecting
    # step of one stream, download of the one-channel image, the host's three equal channels; wall clock, the call is synchronous
    p = capi.multicue_default_params()
    rng = np.random.RandomState(5)
    base = np.repeat(np.repeat(rng.randint(0, 256, (rows // 8, cols // 8, 3)), 8, 0), 8, 1)
    host = [np.clip(base + rng.randint(-2, 3, base.shape), 0, 255).astype(np.uint8) for _ in range(3)]
    for f in host[1:]:
        f[rows // 4:rows // 2, cols // 4:cols // 2] = 200  # a block the model has not seen
    with MultiCueModel(p, n_streams=1) as m:
        for t in range(p.training_period + 1):
            m.process_host(host[0], channels=3)
        for channels in (1, 3):
            ms = []
            for t in range(reps + 3):
                t0 = time.perf_counter()
                m.process_host(host[1 + t % 2], channels=channels)
                ms.append((time.perf_counter() - t0) * 1e3)
            ms = np.array(ms[3:])
            moved_bytes = rows * cols * 4
            print("multicue  1 x %dx%d -> 160x120 host path, %d channel%s out: median %6.3f ms per frame (min %.3f, max %.3f, %d frames): upload %.1f MB + step + download %.1f MB -> %.1f GB/s over the bus"
                  % (cols, rows, channels, "" if channels == 1 else "s", np.median(ms), ms.min(), ms.max(), len(ms), rows * cols * 3 / 1e6, rows * cols / 1e6,
                     moved_bytes / (np.median(ms) * 1e-3) / 1e9))
        assert m.state("overflow")[0] == 0 and m.state("box_overflow")[0] == 0


def run_clip(S=32, rows=1080, cols=1920, kind="sat", steps=48, Ts=(1, 2, 4, 8), algo=None, dense=201.0, label="MOG2"):
    """bgs_process_clip_device on the bench geometry: T frames of every stream per launch, the model held in registers."""
    dev = torch.device("cuda", 0)
    P = 16  # a pool of 16 time steps; S_sat has period 5, so a clip may start at any multiple of 5... the pool is walked cyclically in whole clips
    pool = torch.empty((P, S, rows, cols, 3), dtype=torch.uint8, device=dev)
    gen = synth.s_sat if kind == "sat" else synth.s_surv
    for s in range(S):
        pool[:, s] = gen(P, rows, cols, seed=4321 + s, device=dev)
    px = S * rows * cols
    for T in Ts:
        e = Engine(algo if algo is not None else capi.MOG2, n_streams=S)
        e.set_geometry(rows, cols, 3)
        bits = torch.empty((T, S, rows * cols // 64), dtype=torch.int64, device=dev)
        for t in range(0, 160, T):  # saturate AND age the mixture (every mode of every pixel live on S_sat, weights equalised: steady-state traffic)
            e.process_clip_device(pool[(t % P):(t % P) + T], T, None, None, bits)
        torch.cuda.synchronize()
        for i in range(12):  # auto mode reads its samples after the sync above and may switch kernels (a switch to the filter kernel rebuilds the summaries once): not part of the timing
            t = (160 + i * T) % P
            e.process_clip_device(pool[t:t + T], T, None, None, bits)
        torch.cuda.synchronize()
        e.enable_kernel_timing(True)
        t0 = time.perf_counter()
        for i in range(steps):
            t = (160 + i * T) % P
            e.process_clip_device(pool[t:t + T], T, None, None, bits)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms, n, kname = e.kernel_timing()
        moved = dense / T + 3 + 1 / 8.0
        fused = "clip" in kname or T == 1 or kname == "dp_gmm_kernel"  # one launch per clip call; otherwise T launches, and only the wall clock says what a frame costs
        fms = ms / T if fused else wall * 1e3 / (steps * T)
        print(label + " clip T=%d (%s) %dx%d x%d streams: %-18s %.3f ms per launch, %.3f ms per frame step -> %7.1f Gpix/s = %6.0f 1080p frames/s; "
              "%d B/px/frame algorithmic -> %.2f of 8 TB/s; dense model bytes moved %.1f B/px/frame; wall %.1f Gpix/s"
              % (T, kind, cols, rows, S, kname, ms, fms, px / fms / 1e6, px / fms * 1e3 / (rows * cols), dense + 5, (dense + 5.0) * px / fms / 1e9 / 8.0, moved,
                 px * T * steps / wall / 1e9))
        e.close()


HBM_PEAK_GBPS = 8000.0


def _leg(ms, px, bpp):
    gbps = bpp * px / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    return {"kernel_avg_ms": round(ms, 4), "bytes_per_pixel": bpp, "mpixels_per_s": round(px / ms / 1e3, 1) if ms > 0 else 0.0,
            "achieved_GBps": round(gbps, 1), "frac": round(gbps / HBM_PEAK_GBPS, 4)}


def _cpu_leg(algo, frames_np, warm, label):
    rate, th = cpu_rate(algo, frames_np, warm=warm)
    return {"value": round(rate, 2), "unit": "Mpixels/s", "cores": th, "kind": "port",
            "sample": "%d timed frames %dx%d of stream 0 (same synthetic clip, %d warm-up frames), oracle %s" % (len(frames_np) - warm, frames_np.shape[2], frames_np.shape[1], warm, label)}


def configs_block(device=0, S=8, steps=40, cpu=True):
    """BASELINE configs[2] and configs[3] for bench.py's JSON line (never `value`): kernel time by HIP events on the launch stream,
    algorithmic bytes per pixel of SURVEY.md 8(a), fraction of the 8 TB/s peak, the CPU oracle on a bounded sample beside each."""
    dev = torch.device("cuda", device)
    out = {"note": "BASELINE configs[2] and configs[3], supplementary - never `value`; kernel time = HIP events on the launch stream, bytes per pixel = SURVEY.md 8(a) "
                   "(algorithmic, data-independent where the path is pointwise), frac = of the 8 TB/s HBM peak; cpu = the oracle (port) on a bounded sample of the same frames"}
    # ---- configs[2]: WeightedMovingVarianceBGS + AdaptiveBackgroundLearning, 3840x2160, back to back on the same frames
    rows, cols, T = 2160, 3840, 8
    pool = torch.empty((T, S, rows, cols, 3), dtype=torch.uint8, device=dev)
    for s in range(S):
        pool[:, s] = synth.s_surv(T, rows, cols, seed=4321 + s, device=dev)
    wmv, abl = Engine(capi.WMV, device=device, n_streams=S), Engine(capi.ABL, device=device, n_streams=S)
    for e in (wmv, abl):
        e.set_geometry(rows, cols, 3)
    wmv.set_option(capi.OPT_BORROW_FRAMES, 1)  # the caller's previous frames ARE the history: the algorithmic 10 B/px (the default copies each frame into a private ring)
    fg1 = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    fg2 = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)

    def step23(t):  # (the background image of ABL IS its uint8 state - SURVEY.md 8a a5 counts it once; no separate copy is asked for)
        wmv.process_batch_device(pool[t % T], fg1, None, None)
        abl.process_batch_device(pool[t % T], fg2, None, None)
    for t in range(10):
        step23(t)
    torch.cuda.synchronize()
    wmv.enable_kernel_timing(True), abl.enable_kernel_timing(True)
    t0 = time.perf_counter()
    for t in range(steps):
        step23(10 + t)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    px = S * rows * cols
    ms_w, _, k_w = wmv.kernel_timing()
    ms_a, _, k_a = abl.kernel_timing()
    c2 = {"workload": "WeightedMovingVarianceBGS + AdaptiveBackgroundLearning back to back on the same frames, %d x 3840x2160x3 uint8 S_surv in HBM, one launch per class and step" % S,
          "wmv": dict(_leg(ms_w, px, 10), kernel=k_w), "abl": dict(_leg(ms_a, px, 10), kernel=k_a),
          "both_kernels": _leg(ms_w + ms_a, px, 20), "ms_per_step_wall": round(wall, 4), "frames_4k_per_s": round(S / (wall * 1e-3), 1)}
    if cpu:
        sample = pool[:6, 0].cpu().numpy()
        c2["wmv"]["cpu_baseline"] = _cpu_leg(capi.WMV, sample, 3, "WeightedMovingVarianceBGS, 1 thread")
        c2["abl"]["cpu_baseline"] = _cpu_leg(capi.ABL, sample, 3, "AdaptiveBackgroundLearning, 1 thread")
    wmv.close(), abl.close()
    # the same two classes as ONE fused launch (bgs_group, kernel_fanout.h): one read of the frame and of the shared history
    from tracking_amd.engine import Group
    grp = Group([capi.WMV, capi.ABL], device=device, n_streams=S)
    grp.set_geometry(rows, cols, 3)
    grp.set_option(capi.OPT_BORROW_FRAMES, 1)
    for t in range(10):
        grp.process_batch_device(pool[t % T], [fg1, fg2], None)
    torch.cuda.synchronize()
    grp.enable_kernel_timing(True)
    t0 = time.perf_counter()
    for t in range(steps):
        grp.process_batch_device(pool[(10 + t) % T], [fg1, fg2], None)
    torch.cuda.synchronize()
    wall_g = (time.perf_counter() - t0) / steps * 1e3
    ms_g, _ = grp.kernel_timing()
    # r 3 x 3 (frame, t-1, t-2) + 3 (ABL background) ; w 3 (ABL background) + 1 + 1 (masks) = 17 B/pixel instead of 10 + 10
    c2["fused_group"] = dict(_leg(ms_g, px, 17), kernel="fan_kernel", ms_per_step_wall=round(wall_g, 4), frames_4k_per_s=round(S / (wall_g * 1e-3), 1),
                             speedup_vs_both_kernels=round((ms_w + ms_a) / ms_g, 3) if ms_g > 0 else None,
                             note="bgs_group of the two classes (kernel_fanout.h): ONE launch per step over one read of the frame and of the shared history - "
                                  "17 B/pixel moved (3 frames + ABL state in and out + 2 masks) instead of 10 + 10; outputs bit-identical to the two engines")
    grp.close()
    del pool, fg1, fg2
    out["configs2_wmv_abl_4k"] = c2
    # ---- configs[3]: SuBSENSE (LBSP descriptor path) at 1920x1080: whole frame step, young and aged model; lbsp_kernel alone
    # frames: fresh sensor noise in every frame the model sees (tools/synth.py SurvStreams; round 3 cycled a pool of 8 frames, whose values
    # the 50-sample model then holds exactly): the timed steps run over pools of DISTINCT frames resident in HBM, the untimed ageing
    # generates its frames one by one
    rows, cols, T = 1080, 1920, 36
    src = synth.SurvStreams(S, rows, cols, seed0=4321, device=dev)
    pool = src.pool(T)
    cur = torch.empty((S, rows, cols, 3), dtype=torch.uint8, device=dev)
    e = Engine(capi.SUBSENSE, device=device, n_streams=S)
    t0 = time.perf_counter()
    e.set_geometry(rows, cols, 3)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    e.process_batch_device(pool[0], fg, None, None)  # the first frame initialises the model (refreshModel(1.0): 50 samples per pixel)
    torch.cuda.synchronize()
    init_ms = (time.perf_counter() - t0) * 1e3
    px = S * rows * cols
    c3 = {"workload": "SuBSENSEBGS (LBSP + colour sample consensus, 50 samples per pixel, feedback, post-processing), %d x 1920x1080x3 uint8 S_surv in HBM (fresh sensor noise in every frame), all streams per launch" % S,
          "bytes_per_pixel_note": "data-dependent; SURVEY.md 8(a) a11 gives >= 110 B/pixel (two matching samples, the float maps, frame and mask): `frac` prices the whole step at that floor",
          "first_frame_ms_incl_allocation": round(init_ms, 2)}
    t_seen = 1

    two = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)] if S >= 2 else None

    def step_two_ranges(frames):  # the same batch as two stream ranges, each on a HIP stream of its own (bgs_process_range_device)
        h = S // 2
        e.process_batch_device(frames[:h], fg[:h], None, None, hip_stream=two[0].cuda_stream, first=0, count=h)
        e.process_batch_device(frames[h:], fg[h:], None, None, hip_stream=two[1].cuda_stream, first=h, count=S - h)

    def timed_two_ranges(n):
        """Not a different workload: the S cameras driven as two ranges on two HIP streams, as a host with several capture threads would -
        one range's phase B and post-processing then run beside the other's phase A once the two have drifted apart."""
        nonlocal t_seen
        if two is None:
            return None
        torch.cuda.synchronize()
        for _ in range(3):
            step_two_ranges(pool[t_seen % T])
            t_seen += 1
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        for _ in range(n):
            step_two_ranges(pool[t_seen % T])
            t_seen += 1
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - w0) / n * 1e3
        return {"ms_per_step_wall": round(wall_ms, 4), "frames_1080p_per_s": round(S / (wall_ms * 1e-3), 1),
                "note": "the same %d cameras and frames as ranges [0, %d) and [%d, %d) on two HIP streams, %d steps" % (S, S // 2, S // 2, S, n)}

    def timed(n):
        nonlocal t_seen
        e.enable_kernel_timing(True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        for _ in range(n):
            e.process_batch_device(pool[t_seen % T], fg, None, None)
            t_seen += 1
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - w0) / n * 1e3
        ms, _, kname = e.kernel_timing()
        e.enable_kernel_timing(False)
        # the same steps once more, untimed, with the clock reader running (phase A is bound by vector issue: its time follows the
        # engine clock, and boxes of the pool differ by ~10 % on it)
        from tools.clocks import ClockSampler
        cs = ClockSampler(device)
        cs.start()
        for _ in range(n):
            e.process_batch_device(pool[t_seen % T], fg, None, None)
            t_seen += 1
        torch.cuda.synchronize()
        clk = cs.stop()
        r = _leg(wall_ms, px, 110)
        r["ms_per_step_wall"] = r.pop("kernel_avg_ms")
        r.update({"frames_1080p_per_s": round(S / (wall_ms * 1e-3), 1), "dominant_kernel": kname, "dominant_kernel_avg_ms": round(ms, 4),
                  "foreground_ratio": round(float((fg != 0).float().mean()), 4),
                  "clocks_during_the_same_steps_repeated": {k: clk.get(k) for k in ("engine_clock_MHz", "board_power_W", "samples", "error") if k in clk}})
        return r
    for _ in range(5):
        e.process_batch_device(pool[t_seen % T], fg, None, None)
        t_seen += 1
    c3["young_model"] = dict(timed(30), model_age_frames=6)
    while t_seen < 300:
        e.process_batch_device(src.into(cur), fg, None, None)
        t_seen += 1
    pool[:30] = src.pool(30)
    t_seen = T * 9  # (pool index 0 again: the 30 timed aged steps read 30 frames the model has never seen)
    c3["aged_model"] = dict(timed(30), model_age_frames=300)
    c3["aged_model"]["as_two_ranges_on_two_hip_streams"] = timed_two_ranges(30)
    # model initialisation again (every stream reset: the next frame runs SuBSENSE::initialize - LBSP of the frame, refreshModel(1.0):
    # 50 samples x 16 bytes per pixel written - and then the ordinary step), buffers already allocated
    for s_ in range(S):
        e.reset_stream(s_)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    e.process_batch_device(pool[0], fg, None, None)
    torch.cuda.synchronize()
    reinit_ms = (time.perf_counter() - w0) * 1e3
    model_bytes = S * rows * cols * 50 * 16
    c3["model_initialisation"] = {"first_frame_ms_buffers_allocated": round(reinit_ms, 3), "model_bytes_written": model_bytes,
                                  "note": "one call: initialise + the first ordinary step (~1.7 ms of it); the full refresh writes every record of the model once (ss_refresh_kernel; "
                                          "no separate clear since round 4) - compare calibration.fill_GBps_plain"}
    t_seen = 1
    for _ in range(5):
        e.process_batch_device(pool[t_seen % T], fg, None, None)
        t_seen += 1
    c3["young_model"]["as_two_ranges_on_two_hip_streams"] = timed_two_ranges(30)  # (the re-initialised model at the same age as the leg above)
    e.close()
    from oracle import pyoracle
    lut = pyoracle.lbsp_lut(0.333, 0, 3)
    from tracking_amd.engine import lbsp_describe_batch_device
    imgs = pool[0, :min(S, 16)].contiguous()
    for _ in range(3):
        lbsp_describe_batch_device(imgs, lut)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        lbsp_describe_batch_device(imgs, lut)
    b.record()
    torch.cuda.synchronize()
    c3["lbsp_kernel"] = dict(_leg(a.elapsed_time(b) / 20, imgs.shape[0] * rows * cols, 9), kernel="lbsp_kernel",
                             note="%d frames per launch (bgs_lbsp_describe_batch_device), torch events around 20 calls incl. the output allocation; r 3 + w 6 B/pixel" % imgs.shape[0])
    if cpu:
        sample = pool[:3, 0].cpu().numpy()
        rate, th = cpu_rate(capi.SUBSENSE, sample, warm=1)
        c3["cpu_baseline"] = {"value": round(rate, 3), "unit": "Mpixels/s", "cores": th, "kind": "port",
                              "sample": "2 timed 1920x1080 frames of stream 0 after the initialising frame, oracle SuBSENSE (oracle/subsense_oracle.c), 1 thread"}
    out["configs3_subsense_1080p"] = c3
    del pool
    torch.cuda.empty_cache()
    return out


def kde_scene(T, S, rows, cols, fg_frac, device):
    """T frames of S streams: a static textured scene with fresh +-3 sensor noise in every frame and, when fg_frac > 0, a moving
    saturated box covering fg_frac of the frame (foreground: run_kde learns from box-free frames)."""
    g = torch.Generator(device=device)
    g.manual_seed(77)
    base = torch.randint(30, 200, (S, rows, cols, 3), generator=g, device=device, dtype=torch.int16)
    out = torch.empty((T, S, rows, cols, 3), dtype=torch.uint8, device=device)
    bh, bw = int(rows * fg_frac ** 0.5), int(cols * fg_frac ** 0.5)
    for t in range(T):
        f = base + torch.randint(-3, 4, base.shape, generator=g, device=device, dtype=torch.int16)
        if fg_frac > 0:
            y, x = (t * 37) % (rows - bh), (t * 53) % (cols - bw)
            f[:, y:y + bh, x:x + bw] = torch.tensor([230, 40, 90], device=device, dtype=torch.int16)
        out[t] = f.clamp(0, 255).to(torch.uint8)
    return out


def run_kde(S=8, rows=1080, cols=1920, steps=30, scenes=((("static + noise", 0.0), ("~10 % foreground", 0.1))), count_trips=True):
    """KDE (BGS_KDE) with the reference defaults (50 samples, 10 learning frames, colour ratios): ms per step of S x 1080p for a young
    model (frames 11-40) and one aged ~100 frames, on a static noisy scene and on one with ~10 % foreground; mean density-loop trips
    per pixel from a second, untimed engine with the trip counter on (BGS_KDE_TRIPS=1: one atomic per wave)."""
    dev = torch.device("cuda", 0)
    T = 16
    learn = kde_scene(11, S, rows, cols, 0.0, dev)  # the 10 learning frames + the estimation frame see the empty scene
    for label, frac in scenes:
        pool = kde_scene(T, S, rows, cols, frac, dev)
        fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
        bits = torch.empty((S, rows * cols // 64), dtype=torch.int64, device=dev)
        res = {}
        for counted in ((False, True) if count_trips else (False,)):
            os.environ["BGS_KDE_TRIPS"] = "1" if counted else "0"
            e = Engine(capi.KDE, n_streams=S)
            os.environ.pop("BGS_KDE_TRIPS")
            e.set_geometry(rows, cols, 3)
            t = 0
            for age, upto in (("young", 11), ("aged", 100)):
                while t < upto:
                    e.process_batch_device(learn[t] if t < 11 else pool[t % T], fg, None, bits)
                    t += 1
                torch.cuda.synchronize()
                if counted:
                    t0 = e.get_state("trips", (2,), np.uint64)
                else:
                    e.enable_kernel_timing(True)
                w0 = time.perf_counter()
                for _ in range(steps):
                    e.process_batch_device(pool[t % T], fg, None, bits)
                    t += 1
                torch.cuda.synchronize()
                wall = (time.perf_counter() - w0) / steps * 1e3
                if counted:
                    t1 = e.get_state("trips", (2,), np.uint64)
                    res[age]["mean_trips"] = float(t1[0] - t0[0]) / float(t1[1] - t0[1])
                else:
                    ms, _, kname = e.kernel_timing()
                    e.enable_kernel_timing(False)
                    res[age] = {"wall_ms": wall, "kernel_ms": ms, "fg": float((fg != 0).float().mean())}
            e.close()
        for age, r in res.items():
            print("KDE %-17s %-5s %dx%d x%d streams: %.3f ms/step wall, kde_frame_kernel %.3f ms -> %8.1f Mpix/s; mean trips %s of 50; fg ratio %.3f"
                  % (label, age, cols, rows, S, r["wall_ms"], r["kernel_ms"], S * rows * cols / r["kernel_ms"] / 1e3,
                     "%.2f" % r["mean_trips"] if "mean_trips" in r else "-", r["fg"]))
        del pool
    del learn
    torch.cuda.empty_cache()


def run_dp2(S=8, rows=1080, cols=1920, steps=40, texture_only=False):
    """DPPratiMediodBGS (defaults: history 16, rate 5, threshold 30) and DPTextureBGS at S x 1080p: ms per step by HIP events around
    each step's launches, PratiMediod split into sampled frames (medoid update) and the others (mask only), with a full buffer.
    Bytes per pixel are counted from the layouts of kernel_dp2.h (DRAM traffic if nothing is reused beyond the 3x3 / 15x15
    neighbourhood, which L2 serves); `copy_frac` is the achieved rate over this box's float4 copy rate (bench.py's calibration)."""
    dev = torch.device("cuda", 0)
    px = S * rows * cols
    T = 10
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    base = torch.randint(30, 220, (S, rows, cols, 3), generator=g, device=dev, dtype=torch.int16)
    pool = torch.empty((T, S, rows, cols, 3), dtype=torch.uint8, device=dev)
    bh, bw = rows // 3, cols // 3
    for t in range(T):
        f = base + torch.randint(-4, 5, base.shape, generator=g, device=dev, dtype=torch.int16)
        y, x = (t * 37) % (rows - bh), (t * 53) % (cols - bw)
        f[:, y:y + bh, x:x + bw] = 255 - f[:, y:y + bh, x:x + bw]
        pool[t] = f.clamp(0, 255).to(torch.uint8)
    del base
    copy = capi.calibrate_copy(0, 2 << 30, 0) if not texture_only else float("nan")
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    bits = torch.empty((S, rows * cols // 64), dtype=torch.int64, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]

    def timed(e, t0, n):
        for i in range(n):
            ev[i][0].record()
            e.process_batch_device(pool[(t0 + i) % T], fg, None, bits)
            ev[i][1].record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev[:n]]

    H, rate = 16, 5
    bpp = {"PratiMediod sampled": 16 * 4 + 16 * 2 * 2 + 4 + 4 + 4 + 3 + 1, "PratiMediod other": 4 + 3 + 1, "Texture": 192 + 3 + 2 + 3 + 1 + 64 + 64 + 1}
    legs = {}
    if not texture_only:
        e = Engine(capi.DP_PRATI_MEDIOD, n_streams=S)
        e.set_geometry(rows, cols, 3)
        t = 0
        while t < H * rate + 1:  # fill the buffer
            e.process_batch_device(pool[t % T], fg, None, bits)
            t += 1
        torch.cuda.synchronize()
        t0 = t
        ms = timed(e, t0, steps)
        e.close()
        legs = {"PratiMediod sampled": [m for i, m in enumerate(ms) if (t0 + i) % rate == 0],
                "PratiMediod other": [m for i, m in enumerate(ms) if (t0 + i) % rate != 0]}
    e = Engine(capi.DP_TEXTURE, n_streams=S)
    e.set_geometry(rows, cols, 3)
    timed(e, 0, 3)
    legs["Texture"] = timed(e, 3, steps)
    e.close()
    for label, v in legs.items():
        m = float(np.median(v))
        gbps = bpp[label] * px / (m * 1e-3) / 1e9
        print("%-20s %dx%d x%d streams: %.3f ms/step (median of %d, min %.3f); %d B/px counted -> %.0f GB/s = %.2f of copy %.0f GB/s"
              % (label, cols, rows, S, m, len(v), min(v), bpp[label], gbps, gbps / copy, copy))
    del pool
    torch.cuda.empty_cache()

LB_CLASSES = {"sg": ("LBSimpleGaussian", "LB_SIMPLE_GAUSSIAN"), "fg": ("LBFuzzyGaussian", "LB_FUZZY_GAUSSIAN"), "mog": ("LBMixtureOfGaussians", "LB_MOG"),
              "som": ("LBAdaptiveSOM", "LB_ADAPTIVE_SOM"), "fsom": ("LBFuzzyAdaptiveSOM", "LB_FUZZY_ADAPTIVE_SOM")}


def run_lb(S=8, rows=1080, cols=1920, steps=30, only=None, px_variants=(2, 1), calibrate=True, scenes=(("static + noise", 0.0), ("~10 % foreground", 0.1))):
    """The five package_bgs/lb classes (reference defaults) at S x 1080p, byte mask + background image out: kernel ms per step (HIP
    events around the launch, mean of `steps`) on a static scene with sensor noise and on one with ~10 % foreground, the model aged
    past the SOMs' calibration phase (frame 100 on; for the SOMs also inside it, frames 11 on) - the Gaussian pair with two pixels
    per lane (16 B per lane and plane) and with one (BGS_LB_PX).  Bytes per pixel are the algorithmic ones of kernel_lb.h: frame 3 +
    model read + model written + mask 1 + background 3 (SOMs: + the 3 kept background bytes each way); for MoG and the SOMs the
    dense bound (every slot / all nine neurons) and the least a pixel can move; `copy_frac` is the dense figure's rate over this
    process's float4 copy rate (bench.py's calibration)."""
    dev = torch.device("cuda", 0)
    px = S * rows * cols
    T = 12
    copy = capi.calibrate_copy(0, 2 << 30, 0) if calibrate else float("nan")
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    bg = torch.empty((S, rows, cols, 3), dtype=torch.uint8, device=dev)
    dense = {"sg": 3 + 48 + 48 + 1 + 3, "fg": 3 + 48 + 48 + 1 + 3, "mog": 3 + 172 + 172 + 4, "som": 3 + 216 + 216 + 7 + 3, "fsom": 3 + 216 + 216 + 7 + 3}
    least = {"sg": 103, "fg": 103, "mog": 3 + 60 + 12 + 4, "som": 3 + 216 + 3 + 4, "fsom": 3 + 216 + 96 + 4}
    for label, frac in scenes:
        pool = kde_scene(T, S, rows, cols, frac, dev)
        learn = kde_scene(11, S, rows, cols, 0.0, dev) if frac > 0 else pool
        for key, (name, algo) in LB_CLASSES.items():
            if only and key != only:
                continue
            som = key in ("som", "fsom")
            for pxl in (px_variants if key in ("sg", "fg") else (0,)):
                if pxl:
                    os.environ["BGS_LB_PX"] = str(pxl)
                e = Engine(getattr(capi, algo), n_streams=S)
                os.environ.pop("BGS_LB_PX", None)
                e.set_geometry(rows, cols, 3)
                t = 0
                for phase, upto in ((("calibration", 11), ("online", 100)) if som else (("aged", 100),)):
                    while t < upto:
                        e.process_batch_device(learn[t] if t < 11 else pool[t % T], fg, bg, None)
                        t += 1
                    torch.cuda.synchronize()
                    e.enable_kernel_timing(True)
                    for _ in range(steps):
                        e.process_batch_device(pool[t % T], fg, bg, None)
                        t += 1
                    torch.cuda.synchronize()
                    ms, n, kname = e.kernel_timing()
                    e.enable_kernel_timing(False)
                    gbps = dense[key] * px / (ms * 1e-3) / 1e9
                    print("%-20s %-17s %-11s %s%dx%d x%d streams: %s %.3f ms/step (mean of %d) -> %7.1f Mpix/s; %d B/px dense (least %d) -> %.0f GB/s = %.2f of copy %.0f GB/s; fg ratio %.3f"
                          % (name, label, phase, "%d px/lane " % pxl if pxl else "", cols, rows, S, kname, ms, n, px / ms / 1e3, dense[key], least[key], gbps,
                             gbps / copy, copy, float((fg != 0).float().mean())))
                e.close()
        del pool, learn
        torch.cuda.empty_cache()


def run_lb_clip(S=8, rows=1080, cols=1920, only=None, rounds=5, reps=3, scenes=(("static + noise", 0.0), ("~10 % foreground", 0.1))):
    """Clip calls of the five package_bgs/lb classes at S x 1080p, byte mask + background image out, model aged 100 frames (the SOMs
    online): T = 4 and T = 8 frames per call with BGS_OPT_CLIP_FUSE 1 (one lb_*_clip_kernel launch per call) and 0 (T launches of
    the per-frame kernel: the frame-by-frame path) alternating on the same engine, `rounds` times `reps` calls each.  ms per
    frame = kernel time (HIP events around every launch) over the frames; the median of the rounds, and the spread (min .. max) of
    the unfused rounds, which is what a gain has to exceed.  B/pixel/frame: frame 3 + mask 1 + background 3 per frame, the model
    read and written once per call (dense bound for MoG and the SOMs, SOMs + the 3 kept background bytes each way)."""
    dev = torch.device("cuda", 0)
    px = S * rows * cols
    model = {"sg": 96, "fg": 96, "mog": 344, "som": 438, "fsom": 438}
    for label, frac in scenes:
        pool = kde_scene(12, S, rows, cols, frac, dev)
        learn = kde_scene(11, S, rows, cols, 0.0, dev) if frac > 0 else pool
        fg = torch.empty((8, S, rows, cols), dtype=torch.uint8, device=dev)
        bg = torch.empty((8, S, rows, cols, 3), dtype=torch.uint8, device=dev)
        for key, (name, algo) in LB_CLASSES.items():
            if only and key != only:
                continue
            e = Engine(getattr(capi, algo), n_streams=S)
            e.set_geometry(rows, cols, 3)
            for t in range(100):
                e.process_batch_device(learn[t] if t < 11 else pool[t % 12], None, None, None)
            for T in (4, 8):
                slab = pool[:T]
                ms = {1: [], 0: []}
                kn = {}
                for _ in range(rounds):
                    for fuse in (1, 0):
                        e.set_option(capi.OPT_CLIP_FUSE, fuse)
                        torch.cuda.synchronize()
                        e.enable_kernel_timing(True)
                        for _ in range(reps):
                            e.process_clip_device(slab, T, fg, bg)
                        torch.cuda.synchronize()
                        avg, n, kn[fuse] = e.kernel_timing()
                        e.enable_kernel_timing(False)
                        assert n == reps * (1 if fuse else T) and ("clip" in kn[fuse]) == bool(fuse), (n, kn[fuse])
                        ms[fuse].append(avg * n / (reps * T))
                f, u = float(np.median(ms[1])), float(np.median(ms[0]))
                spread = max(ms[0]) - min(ms[0])
                bpf = model[key] / T + 7
                print("%-20s %-17s clip T=%d %dx%d x%d streams: fused %s %.3f ms/frame (min %.3f max %.3f), unfused %s %.3f ms/frame (min %.3f max %.3f, spread %.3f); "
                      "gain %.3f ms = x%.2f -> %s; fused %.1f B/px/frame -> %.0f GB/s"
                      % (name, label, T, cols, rows, S, kn[1], f, min(ms[1]), max(ms[1]), kn[0], u, min(ms[0]), max(ms[0]), spread, u - f, u / f,
                         "faster than the spread" if u - f > spread else "NOT faster than the spread", bpf, bpf * px / (f * 1e-3) / 1e9))
            e.close()
        del pool, learn, fg, bg
        torch.cuda.empty_cache()


def run_vumeter(S=8, rows=1080, cols=1920, steps=30, age=60):
    """VuMeter (reference defaults: 32 bins, alpha 0.995) at S x 1080p, byte mask + background image out, for the three kernel variants
    in one process on the same frames: the model kernel's ms per step (HIP events around the launch, mean of `steps`) and the wall ms
    per step with the post-filter off and on (erode + median: two more launches), after `age` frames.  Scenes: S_surv (tools/synth.py),
    fresh uniform noise, where every bin of every pixel becomes live, and S_smooth (S_surv's boxes over a low-frequency background).  Bytes per pixel are the model's own accounting from the
    histograms of stream 0 after the run: L = live bins per pixel, U = bins live in at least one of a wave's 64 pixels (U16: of
    16 consecutive pixels, one 64-byte sector of a plane);
      dense 3 + 128 + 128 + 4;  live-bin 3 + 4 L + 4 U + 8 (bitmap) + 4;  live-bin, masked stores 3 + 4 L + 4 L + 8 + 4
    (the 4: background byte read and written, background image, mask).  `copy_frac` is that figure's rate over this process's
    float4 copy rate."""
    dev = torch.device("cuda", 0)
    px = S * rows * cols
    T = 12
    copy = capi.calibrate_copy(0, 2 << 30, 0)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    bg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    for label in ("S_surv", "uniform noise", "S_smooth"):
        if label == "S_surv":
            pool = synth.SurvStreams(S, rows, cols, seed0=4321, device=dev).pool(T)
        elif label == "S_smooth":  # not asked of the class; shows what the live-bin kernels gain when neighbours share bins
            pool = torch.stack([synth.s_smooth(T, rows, cols, seed=777 + k, device=dev) for k in range(S)], 1)
        else:
            pool = torch.randint(0, 256, (T, S, rows, cols, 3), generator=g, device=dev, dtype=torch.uint8)
        for mode, name in ((0, "dense"), (1, "live-bin"), (2, "live-bin, masked stores")):
            os.environ["BGS_VU_SPARSE"] = str(mode)
            e = Engine(capi.VUMETER, n_streams=S)
            os.environ.pop("BGS_VU_SPARSE", None)
            e.set_geometry(rows, cols, 3)
            t = 0
            res = {}
            for filt in (0, 1):
                p = capi.default_params(capi.VUMETER)
                p.vu_enable_filter = filt
                e.set_params(p)
                while t < age * (filt + 1):  # the noise scene ages on frames of its own, so that every bin of every pixel gets hit
                    e.process_batch_device(pool[t % T] if label != "uniform noise" else torch.randint(0, 256, pool[0].shape, generator=g, device=dev, dtype=torch.uint8), fg, bg, None)
                    t += 1
                torch.cuda.synchronize()
                e.enable_kernel_timing(True)
                w0 = time.perf_counter()
                for _ in range(steps):
                    e.process_batch_device(pool[t % T], fg, bg, None)
                    t += 1
                torch.cuda.synchronize()
                wall = (time.perf_counter() - w0) / steps * 1e3
                ms, n, kname = e.kernel_timing()
                e.enable_kernel_timing(False)
                res[filt] = (ms, wall, n, kname)
            h = torch.from_numpy(e.get_state("hist", (32, rows * cols), np.float32)) != 0
            L = float(h.sum(0).float().mean())
            U = float(h.reshape(32, -1, 64).any(2).sum(0).float().mean())
            U16 = float(h.reshape(32, -1, 16).any(2).sum(0).float().mean())
            bpp = {0: 3 + 128 + 128 + 4, 1: 3 + 4 * L + 4 * U + 8 + 4, 2: 3 + 8 * L + 8 + 4}[mode]
            sect = {0: bpp, 1: 3 + 4 * U16 + 4 * U + 8 + 4, 2: 3 + 8 * U16 + 8 + 4}[mode]  # memory moves 64-byte sectors, not lanes' dwords
            ms = res[0][0]
            gbps = bpp * px / (ms * 1e-3) / 1e9
            print("VuMeter %-14s %-24s %dx%d x%d streams: %s %.3f ms/step filter off (%.3f with the filter on; mean of %d) -> %7.1f Mpix/s; wall %.3f / %.3f ms/step; "
                  "L %.2f live bins/px, U16 %.2f per 16 px, U %.2f per wave; %.1f B/px requested (%.1f in 64-byte sectors) -> %.0f GB/s = %.2f of copy %.0f GB/s (sectors: %.2f); fg ratio %.3f"
                  % (label, name, cols, rows, S, res[0][3], ms, res[1][0], res[0][2], px / ms / 1e3, res[0][1], res[1][1], L, U16, U, bpp, sect, gbps, gbps / copy, copy, sect * px / (ms * 1e-3) / 1e9 / copy,
                     float((fg != 0).float().mean())))
            e.close()
        del pool
        torch.cuda.empty_cache()


def run_fuzzy(S=8, rows=1080, cols=1920, steps=20, only=None, calibrate=True):
    """The two fuzzy integrals (reference defaults) at S x 1080p on S_surv, byte mask + background image out: ms per learning step (one
    launch) and per detecting step (seven launches: HIP events around the whole step, mean of `steps`) and the wall ms per step.
    Bytes per pixel are the kernels' own accounting of what a detecting step requests (kernel_fuzzy.h): prep 3 + 12 in, 8 out; pixel
    3 + 12 + 8 in, 12 + 1 out; scan 1 in; apply 1 + 12 in, 4 out; median 4 in, 4 + 1 out; update 4 + 3 + 12 in, 12 + 3 out = 120; a
    learning step 3 + 12 in, 12 out = 27.  `copy_frac` is that figure's rate over this process's float4 copy rate."""
    dev = torch.device("cuda", 0)
    px = S * rows * cols
    T = 8
    copy = capi.calibrate_copy(0, 2 << 30, 0) if calibrate else float("nan")
    pool = synth.SurvStreams(S, rows, cols, seed0=4321, device=dev).pool(T)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    bg = torch.empty((S, rows, cols, 3), dtype=torch.uint8, device=dev)
    for algo, name in ((capi.FUZZY_SUGENO, "FuzzySugenoIntegral"), (capi.FUZZY_CHOQUET, "FuzzyChoquetIntegral")):
        if only and name != only:
            continue
        e = Engine(algo, n_streams=S)
        e.set_geometry(rows, cols, 3)
        res = {}
        t = 0
        for phase, ftl, bpp in (("learning", 1 << 30, 27.0), ("detecting", 0, 120.0)):
            e.set_fuzzy_params(frames_to_learn=ftl)
            for _ in range(4):
                e.process_batch_device(pool[t % T], fg, bg, None)
                t += 1
            torch.cuda.synchronize()
            e.enable_kernel_timing(True)
            w0 = time.perf_counter()
            for _ in range(steps):
                e.process_batch_device(pool[t % T], fg, bg, None)
                t += 1
            torch.cuda.synchronize()
            wall = (time.perf_counter() - w0) / steps * 1e3
            ms, n, kname = e.kernel_timing()
            e.enable_kernel_timing(False)
            gbps = bpp * px / (ms * 1e-3) / 1e9
            res[phase] = (ms, wall, n, gbps)
            print("%-20s %-9s %dx%d x%d streams: %.3f ms/step (%s; mean of %d) -> %7.1f Mpix/s; wall %.3f ms/step; %.0f B/px requested -> %.0f GB/s = %.2f of copy %.0f GB/s; fg ratio %.3f"
                  % (name, phase, cols, rows, S, ms, kname, n, px / ms / 1e3, wall, bpp, gbps, gbps / copy, copy, float((fg != 0).float().mean()) if ftl == 0 else 0.0))
        e.close()


def run_t2f(S=8, rows=1080, cols=1920, steps=30, clips=10, age=40):
    """T2FGMM_UM / T2FGMM_UV beside DPGrimsonGMM (the yardstick: the same control flow with one plane per mode more) in one process,
    reference defaults (K = 3), on S_surv, byte mask out: kernel ms per single-frame step (mean of `steps`) and per frame of a
    T = 8 clip launch (mean of `clips` launches / 8).  `dense` is what a step requests when every mode is live and every field
    changes: K * F * 4 bytes of model in and out, the count byte, 3 of frame, 1 of mask; the kernels store only fields whose bits
    changed, so the real traffic is below it.  copy_frac is that figure's rate over this process's float4 copy rate."""
    dev = torch.device("cuda", 0)
    px = S * rows * cols
    T = 8
    copy = capi.calibrate_copy(0, 2 << 30, 0)
    pool = synth.SurvStreams(S, rows, cols, seed0=4321, device=dev).pool(2 * T)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    cfg = torch.empty((T, S, rows, cols), dtype=torch.uint8, device=dev)
    # two rounds over the three classes, a fresh engine each time: the second round shows the spread inside one process
    for algo, name, F in ((capi.DP_GRIMSON_GMM, "DPGrimsonGMMBGS", 6), (capi.T2FGMM_UM, "T2FGMM_UM", 5), (capi.T2FGMM_UV, "T2FGMM_UV", 5)) * 2:
        e = Engine(algo, n_streams=S)
        e.set_geometry(rows, cols, 3)
        K = e.params.dp_gaussians if algo == capi.DP_GRIMSON_GMM else e.get_t2f_params().gaussians  # the classes' own defaults: the comparison is at equal K or says so
        dense = 2 * K * F * 4 + 1 + 3 + 1
        t = 0
        for _ in range(age):
            e.process_batch_device(pool[t % (2 * T)], fg, None, None)
            t += 1
        torch.cuda.synchronize()
        e.enable_kernel_timing(True)
        for _ in range(steps):
            e.process_batch_device(pool[t % (2 * T)], fg, None, None)
            t += 1
        torch.cuda.synchronize()
        ms, n, kname = e.kernel_timing()
        ratio = float((fg != 0).float().mean())
        e.enable_kernel_timing(False)
        e.enable_kernel_timing(True)
        for i in range(clips):
            e.process_clip_device(pool[(i % 2) * T:(i % 2) * T + T], T, cfg, None, None)
        torch.cuda.synchronize()
        cms, cn, cname = e.kernel_timing()
        gbps = dense * px / (ms * 1e-3) / 1e9
        print("%-16s K=%d %dx%d x%d streams: %.3f ms/step (%s; mean of %d) -> %7.1f Mpix/s; dense %d B/px -> %.0f GB/s = %.2f of copy %.0f GB/s; clip T=8: %.3f ms/launch = %.3f ms/frame (%s; mean of %d); fg ratio %.3f"
              % (name, K, cols, rows, S, ms, kname, n, px / ms / 1e3, dense, gbps, gbps / copy, copy, cms, cms / T, cname, cn, ratio))
        e.close()


def run_eigen(S=8, rows=1080, cols=1920, steps=30):
    """DPEigenbackgroundBGS at the reference defaults beside DPGrimsonGMM (a yardstick from the same package, timed in the same
    process) on S_surv, byte mask out.  Per engine: ms per detecting step (kernel timing over project + coeff + reconstruct, mean of
    `steps`), the one-off build at frame H (the frame-H call between two events on the launch stream, less one detecting step), and
    what 2 * 12 * M + 2 * 12 + 2 * 3 + 1 bytes per pixel (both reads of the eigenvectors and of avg, both of the frame, the mask) come
    to as a rate over this process's float4 copy rate.  S streams and then one stream alone: a single 1080p stream's eigenvectors
    (249 MB at M = 10) are within reach of the 256 MiB Infinity Cache between the two reads, eight streams' are not."""
    dev = torch.device("cuda", 0)
    copy = capi.calibrate_copy(0, 2 << 30, 0)
    for streams in (S, 1):
        px = streams * rows * cols
        e = Engine(capi.DP_EIGENBACKGROUND, n_streams=streams)
        e.set_geometry(rows, cols, 3)
        q = e.get_eigen_params()
        H, M = q.history_size, q.embedded_dim
        pool = synth.SurvStreams(streams, rows, cols, seed0=4321, device=dev).pool(H + 4)
        fg = torch.empty((streams, rows, cols), dtype=torch.uint8, device=dev)
        for t in range(H):
            e.process_batch_device(pool[t], fg, None, None)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e.process_batch_device(pool[H], fg, None, None)  # builds the model, then detects
        b.record()
        torch.cuda.synchronize()
        first_ms = a.elapsed_time(b)
        for t in range(3):
            e.process_batch_device(pool[H + 1 + t], fg, None, None)
        torch.cuda.synchronize()
        e.enable_kernel_timing(True)
        for t in range(steps):
            e.process_batch_device(pool[H + t % 4], fg, None, None)
        torch.cuda.synchronize()
        ms, n, kname = e.kernel_timing()
        ratio = float((fg != 0).float().mean())
        bpp = 2 * 12 * M + 2 * 12 + 2 * 3 + 1
        gbps = bpp * px / (ms * 1e-3) / 1e9
        print("%-22s H=%d M=%d %dx%d x%d streams: %.3f ms/step (%s; mean of %d) = %.3f ms/stream -> %7.1f Mpix/s; %d B/px -> %.0f GB/s = %.2f of copy %.0f GB/s; build at frame H: %.3f ms (frame-H call %.3f ms); fg ratio %.3f"
              % ("DPEigenbackgroundBGS", H, M, cols, rows, streams, ms, kname, n, ms / streams, px / ms / 1e3, bpp, gbps, gbps / copy, copy, first_ms - ms, first_ms, ratio))
        e.close()
        del pool
    g = Engine(capi.DP_GRIMSON_GMM, n_streams=S)
    g.set_geometry(rows, cols, 3)
    pool = synth.SurvStreams(S, rows, cols, seed0=4321, device=dev).pool(8)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    for t in range(40):
        g.process_batch_device(pool[t % 8], fg, None, None)
    torch.cuda.synchronize()
    g.enable_kernel_timing(True)
    for t in range(steps):
        g.process_batch_device(pool[t % 8], fg, None, None)
    torch.cuda.synchronize()
    ms, n, kname = g.kernel_timing()
    print("%-22s K=%d %dx%d x%d streams: %.3f ms/step (%s; mean of %d)" % ("DPGrimsonGMMBGS", g.params.dp_gaussians, cols, rows, S, ms, kname, n))
    g.close()


def run_imbs(S=8, rows=1080, cols=1920):
    """IndependentMultimodalBGS at the wrapper's defaults (fps 10, numSamples 30, a sample every 5th frame, the first model at frame
    145, the next ones every 145 frames: a build does not move prev_bg_frame_time) on S_surv, mask and background out.  Every step enqueues the same launches; what differs is what the sample kernel finds in
    its stream's control block, so the three kinds of step are timed apart, each call between two events on the launch stream:
    detect-only (no createBg), sampling (createBg(k), k < 29) and build (createBg(29)), each before and after the first model; which
    kind a step was is read from the stream's control block on the device (bg_frame_counter before and after the call).
    Bytes per pixel are the layout's: 4 per bin and model slot, 12 for the persistence map, bgSample and bgImage, 21 of per-frame
    scratch (labels, planes, two labellings, areas).  A learning step costs every launch on all-zero planes with no model read; the
    kernel-timing window is the detect kernel alone; the split by kernel is a kernel trace's to give.  The CPU
    figure is the numpy restatement (tests/imbs_numpy.py, the quad form of the area filter) on a 120 x 160 crop, per pixel."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import imbs_numpy as im
    dev = torch.device("cuda", 0)
    copy = capi.calibrate_copy(0, 2 << 30, 0)
    px = S * rows * cols
    e = Engine(capi.IMBS, n_streams=S)
    e.set_geometry(rows, cols, 3)
    q = e.get_imbs_params()
    N, M = q.numSamples, q.numSamples // q.minBinHeight
    pool = synth.SurvStreams(S, rows, cols, seed0=4321, device=dev).pool(8)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    bg = torch.empty((S, rows, cols, 3), dtype=torch.uint8, device=dev)
    every = int(round(q.samplingPeriod / (1000. / q.fps)))
    total = 3 * every * (N - 1) + every  # the learning phase and two more models: a model takes every (N - 1) frames
    kinds = {}
    before = e.get_state("control", (10,), np.float64)
    for t in range(total):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e.process_batch_device(pool[t % 8], fg, bg, None)
        b.record()
        torch.cuda.synchronize()
        # what the step did, from the device's own control block (stream 0; the streams are in lock-step): bg_frame_counter went up
        # by one = createBg(k) on a fresh sample, fell to 0 = the build createBg(numSamples - 1), stayed = no createBg
        after = e.get_state("control", (10,), np.float64)
        phase = "detecting" if before[9] else "learning"  # bgModel[0].isValid[0] when the step began
        kind = "sample" if after[3] == before[3] + 1 else "build" if before[3] == before[4] - 1 and after[3] == 0 else "detect-only"
        assert kind != "detect-only" or after[3] == before[3]
        if t > 2:
            kinds.setdefault((phase, kind), []).append(a.elapsed_time(b))
        before = after
    ctl = e.get_state("control", (10,), np.float64)
    ratio = float((fg == 255).float().mean())
    state_bpp = 4 * N + 4 * M + 12
    print("IndependentMultimodalBGS numSamples=%d maxBgBins=%d %dx%d x%d streams, %d steps; state %d B/px + 21 B/px scratch; copy %.0f GB/s; control after the last step %s; 255 ratio %.3f"
          % (N, M, cols, rows, S, total, state_bpp, copy, ctl.tolist(), ratio))
    for key in sorted(kinds):
        v = np.array(kinds[key])
        print("  %-10s %-12s %4d steps: median %.3f ms (min %.3f, max %.3f) = %.3f ms/stream -> %7.1f Mpix/s" % (key[0], key[1], len(v), np.median(v), v.min(), v.max(), np.median(v) / S, px / np.median(v) / 1e3))
    det = float(np.median(kinds[("detecting", "detect-only")]))
    # what a detect-only step must move: the frame, model slots up to the first invalid one (at least one), the persistence map, the
    # label and the 255-plane, then the filter's scratch and the images out
    print("  detect-only against the copy rate: %d B/px of state + scratch if every slot were read = %.0f GB/s = %.2f of copy" % (state_bpp + 21, (state_bpp + 21) * px / (det * 1e-3) / 1e9, (state_bpp + 21) * px / (det * 1e-3) / 1e9 / copy))
    e.enable_kernel_timing(True)
    for t in range(10):
        e.process_batch_device(pool[t % 8], fg, bg, None)
    torch.cuda.synchronize()
    ms, n, kname = e.kernel_timing()
    lrn = float(np.median(kinds[("learning", "detect-only")]))
    builds = sorted(kinds.get(("learning", "build"), []) + kinds.get(("detecting", "build"), []))
    print("  every build step: %s ms" % ", ".join("%.3f" % v for v in builds))
    print("  %s alone: %.3f ms (mean of %d); a learning step (every launch on all-zero planes, no model read): %.3f ms; a detecting step: %.3f ms" % (kname, ms, n, lrn, det))
    e.close()
    small = synth.SurvStreams(1, 120, 160, seed0=4321, device=dev).pool(8).cpu().numpy()[:, 0]
    m = im.Model(dict(im.DEFAULTS, **im.FAST), 120, 160, area_filter=im.area_filter_quads)
    for t in range(8):
        m.apply(small[t % 8])
    t0 = time.perf_counter()
    for t in range(4):
        m.apply(small[t % 8])
    cpu = (time.perf_counter() - t0) / 4
    print("  numpy restatement (numSamples 6, quad form) on 120 x 160: %.1f ms per frame = %.2f us/pixel; the engine's detecting step: %.5f us/pixel" % (cpu * 1e3, cpu * 1e6 / (120 * 160), det * 1e3 / px))


def run_multilayer(S=8, rows=1080, cols=1920, steps=30):
    """MultiLayerBGS at the wrapper's defaults (five modes, a 9 x 9 Gaussian) on S_surv, mask and background out.  Every step is two
    launches: ml_model_kernel (kernel timing: events around that launch alone) and ml_smooth_kernel (what is left of the step, which is
    timed between two events on the launch stream with the host far ahead).  The model is aged 40 frames first, past the frame at which
    a matched mode gets its layer (14).  Bytes per pixel are the layout's: 67 dword planes of model, the raw and the smoothed distance
    map; what a step moves depends on how many modes a pixel lists (13 planes read per listed mode, 2 + 2 per listed mode + 11 written),
    so the rate against this process's own copy rate is given for the mean number of listed modes read back from the state."""
    dev = torch.device("cuda", 0)
    copy = capi.calibrate_copy(0, 2 << 30, 0)
    px = S * rows * cols
    e = Engine(capi.MULTILAYER, n_streams=S)
    e.set_geometry(rows, cols, 3)
    pool = synth.SurvStreams(S, rows, cols, seed0=4321, device=dev).pool(8)
    fg = torch.empty((S, rows, cols), dtype=torch.uint8, device=dev)
    bg = torch.empty((S, rows, cols, 3), dtype=torch.uint8, device=dev)
    for t in range(40):
        e.process_batch_device(pool[t % 8], fg, bg, None)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(steps):
        e.process_batch_device(pool[t % 8], fg, bg, None)
    b.record()
    torch.cuda.synchronize()
    step = a.elapsed_time(b) / steps
    e.enable_kernel_timing(True)
    for t in range(steps):
        e.process_batch_device(pool[t % 8], fg, bg, None)
    torch.cuda.synchronize()
    ms, n, kname = e.kernel_timing()
    order = e.get_state("order", (rows * cols, 7), np.uint8)
    listed = float(order[:, 0].mean())
    ratio = float((fg != 0).float().mean())
    state_bpp = 4 * 67 + 8
    moved = 3 * 7 + 8 + 13 * 4 * listed + (2 + 2 * listed + 11) * 4 + 4 + 3 + 4 * 2 + 4 + 1  # frame and six neighbours, header, modes, write-back, raw, background, the blur
    print("MultiLayerBGS defaults %dx%d x%d streams, %d steps after 40: %.3f ms/step = %.3f ms/stream -> %7.1f Mpix/s; %s %.3f ms (mean of %d), the rest of the step (ml_smooth_kernel) %.3f ms"
          % (cols, rows, S, steps, step, step / S, px / step / 1e3, kname, ms, n, step - ms))
    print("  state %d B/px (67 dword planes + raw + smoothed distance); %.2f modes listed per pixel (stream 0) -> about %.0f B/px moved per step = %.0f GB/s = %.2f of this process's copy rate %.0f GB/s; fg ratio %.3f"
          % (state_bpp, listed, moved, moved * px / (step * 1e-3) / 1e9, moved * px / (step * 1e-3) / 1e9 / copy, copy, ratio))
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--only", default="", help="subsense: just the SuBSENSE lines")
    args = ap.parse_args()
    S = args.streams
    if args.only == "kde":
        run_kde(S)
        return
    if args.only == "dp2":
        run_dp2(S)
        return
    if args.only == "lb":
        run_lb(S)
        run_lb_clip(S)
        return
    if args.only == "lb_clip":  # the clip legs alone
        run_lb_clip(S)
        return
    if args.only == "vumeter":
        run_vumeter(S)
        return
    if args.only == "fuzzy":
        run_fuzzy(S)
        return
    if args.only == "t2f":
        run_t2f(S)
        return
    if args.only == "eigen":
        run_eigen(S)
        return
    if args.only == "imbs":
        run_imbs(S)
        return
    if args.only == "multilayer":
        run_multilayer(S)
        return
    if args.only == "canny":
        run_canny()
        return
    if args.only == "lbpmrf_mask":
        run_lbpmrf_mask()
        return
    if args.only == "multicue":
        run_multicue()
        return
    if args.only in ("fuzzy_choquet", "fuzzy_sugeno"):
        run_fuzzy(S, steps=5, only="FuzzyChoquetIntegral" if args.only == "fuzzy_choquet" else "FuzzySugenoIntegral", calibrate=False)
        return
    if args.only.startswith("lb_") and args.only[3:] in LB_CLASSES:  # one class, the foreground scene, short legs, no calibration: for counter passes
        run_lb(S, steps=5, only=args.only[3:], px_variants=(0,), calibrate=False, scenes=(("~10 % foreground", 0.1),))
        return
    if args.only == "dp2_tex":  # Texture only, short leg, no calibration: for counter passes
        run_dp2(S, steps=5, texture_only=True)
        return
    if args.only in ("kde_static", "kde_fg"):  # one scene, short legs, no trip counter: for counter passes
        run_kde(S, steps=5, scenes=((("static + noise", 0.0),) if args.only == "kde_static" else (("~10 % foreground", 0.1),)), count_trips=False)
        return
    if args.only == "subsense":
        run_subsense(2)
        run_subsense(2, kind="smooth")
        return
    if args.only == "byte":  # the byte-stream kernels only, no CPU leg (kernel iteration)
        run(capi.WMV, "WeightedMovingVarianceBGS", 2160, 3840, S, 10, cpu_frames=0)
        run(capi.WMV, "WeightedMovingVarianceBGS (S_sat: every pixel moves)", 2160, 3840, S, 10, cpu_frames=0, kind="sat")
        run(capi.ABL, "AdaptiveBackgroundLearning", 2160, 3840, S, 10, borrow=False, cpu_frames=0)
        run(capi.ABL, "AdaptiveBackgroundLearning (S_sat)", 2160, 3840, S, 10, borrow=False, cpu_frames=0, kind="sat")
        run(capi.WMM, "WeightedMovingMeanBGS (+bg)", 2160, 3840, S, 13, want_bg=True, cpu_frames=0)
        run(capi.WMM, "WeightedMovingMeanBGS (mask only)", 2160, 3840, S, 10, cpu_frames=0)
        run(capi.FRAME_DIFF, "FrameDifferenceBGS", 2160, 3840, S, 7, cpu_frames=0)
        run(capi.SIGMA_DELTA, "SigmaDeltaBGS", 2160, 3840, S, 16, borrow=False, cpu_frames=0)
        run(capi.ASBL, "AdaptiveSelectiveBackgroundLearning", 2160, 3840, S, 6, borrow=False, cpu_frames=0)
        det = capi.default_params(capi.ASBL)
        det.learning_frames = 4
        run(capi.ASBL, "ASBL (detection phase)", 2160, 3840, S, 6, borrow=False, cpu_frames=0, params=det)
        return
    if args.only in ("clip8sat", "clip8surv"):  # one short leg, for counter passes
        run_clip(kind=args.only[5:], steps=6, Ts=(8,))
        return
    if args.only == "clip":
        run_clip(kind="sat")
        run_clip(kind="surv")
        return
    if args.only == "clipdp":  # package_bgs/dp GMMs (K = 3: 60 / 72 B/px of model + the count byte)
        run_clip(S=16, kind="sat", algo=capi.DP_ZIVKOVIC_AGMM, dense=122.0, label="DPZivkovicAGMM")
        run_clip(S=16, kind="surv", algo=capi.DP_ZIVKOVIC_AGMM, dense=122.0, label="DPZivkovicAGMM")
        run_clip(S=16, kind="sat", algo=capi.DP_GRIMSON_GMM, dense=146.0, label="DPGrimsonGMM")
        return
    if args.only == "clipfd":  # history classes: inside a clip the clip's own frames are the history (no per-frame copy into the ring)
        for algo, label in ((capi.FRAME_DIFF, "FrameDifference"), (capi.WMV, "WeightedMovingVariance")):
            run_clip(S=8, rows=2160, cols=3840, kind="surv", algo=algo, dense=3.0, label=label, Ts=(1, 4, 8))
        return
    if args.only == "clip1":  # MixtureOfGaussianV1BGS clips (16 streams: 320 B/px of model)
        run_clip(S=16, kind="sat", algo=capi.MOG1, dense=320.0, label="MOG1")
        run_clip(S=16, kind="surv", algo=capi.MOG1, dense=320.0, label="MOG1")
        return
    if args.only == "byte32":  # the same byte-stream kernels with 32 x 4K per launch (2.6 GB): how much of the gap to 0.79 is launch size
        run(capi.WMV, "WeightedMovingVarianceBGS", 2160, 3840, 32, 10, cpu_frames=0, steps=30)
        run(capi.ABL, "AdaptiveBackgroundLearning", 2160, 3840, 32, 10, borrow=False, cpu_frames=0, steps=30)
        run(capi.FRAME_DIFF, "FrameDifferenceBGS", 2160, 3840, 32, 7, cpu_frames=0, steps=30)
        return
    if args.only in ("mog1", "mog1sat", "mog1surv"):  # MixtureOfGaussianV1BGS update kernel on both inputs (no CPU leg: kernel iteration / counter passes)
        if args.only != "mog1surv":
            run(capi.MOG1, "MixtureOfGaussianV1BGS (S_sat)", 1080, 1920, 16, 324, borrow=False, kind="sat", cpu_frames=0)
        if args.only != "mog1sat":
            run(capi.MOG1, "MixtureOfGaussianV1BGS (S_surv)", 1080, 1920, 16, 324, borrow=False, cpu_frames=0)
        return
    if args.only == "lbsp":
        run_lbsp()
        return
    if args.only == "pipeline":
        run_pipeline()
        return
    if args.only == "group":  # BASELINE configs[2] as one fused launch (bgs_group of WMV + ABL, kernel_fanout.h) - for counter passes
        from tracking_amd.engine import Group
        dev = torch.device("cuda", 0)
        rows, cols, T = 2160, 3840, 8
        pool = torch.empty((T, S, rows, cols, 3), dtype=torch.uint8, device=dev)
        for s_ in range(S):
            pool[:, s_] = synth.s_surv(T, rows, cols, seed=4321 + s_, device=dev)
        fg1, fg2 = (torch.empty((S, rows, cols), dtype=torch.uint8, device=dev) for _ in range(2))
        grp = Group([capi.WMV, capi.ABL], device=0, n_streams=S)
        grp.set_geometry(rows, cols, 3)
        grp.set_option(capi.OPT_BORROW_FRAMES, 1)
        for t in range(10):
            grp.process_batch_device(pool[t % T], [fg1, fg2], None)
        torch.cuda.synchronize()
        grp.enable_kernel_timing(True)
        for t in range(40):
            grp.process_batch_device(pool[(10 + t) % T], [fg1, fg2], None)
        torch.cuda.synchronize()
        ms, _ = grp.kernel_timing()
        px = S * rows * cols
        print("WMV + ABL as one bgs_group       %dx%d x%d streams: kernel fan_kernel %.4f ms -> %.1f Mpix/s  %.1f GB/s algorithmic (17 B/px) = %.1f%% of 8 TB/s"
              % (cols, rows, S, ms, px / ms / 1e3, 17 * px / ms / 1e6, 17 * px / ms / 1e6 / 80.0))
        grp.close()
        return
    if args.only in ("gmg", "gmgsat"):  # GMG in normal operation (counter passes / kernel iteration)
        pg = capi.default_params(capi.GMG)
        pg.gmg_init_frames = 4
        run(capi.GMG, "GMG (data-dependent traffic)", 1080, 1920, 8, 16, borrow=False, cpu_frames=0, params=pg, kind="sat" if args.only == "gmgsat" else "surv")
        return
    if args.only == "dp":
        run_dp()
        return
    if args.only in ("dpzsat", "dpzsurv", "dpgsat", "dpgsurv"):  # one dp GMM leg (counter passes)
        algo, bpp, nm = (capi.DP_ZIVKOVIC_AGMM, 126, "DPZivkovicAGMMBGS") if args.only[2] == "z" else (capi.DP_GRIMSON_GMM, 150, "DPGrimsonGMMBGS")
        kind = args.only[3:]
        run(algo, "%s (K=3, S_%s)" % (nm, kind), 1080, 1920, 16, bpp, borrow=False, kind=kind, cpu_frames=0)
        return
    if args.only == "cc":
        run_cc()
        return
    if args.only == "lobster":
        run_subsense(8, algo=capi.LOBSTER, label="LOBSTERBGS")
        run_subsense(8, kind="smooth", algo=capi.LOBSTER, label="LOBSTERBGS")
        return
    if args.only == "subsense8":
        run_subsense(8)
        return
    if args.only == "driverconfigs":  # the configs[2] / configs[3] block exactly as bench.py puts it into the driver's line (no CPU legs): A/B scripts
        out = configs_block(S=S, cpu=False)
        c3 = out["configs3_subsense_1080p"]
        for k in ("young_model", "aged_model"):
            clk = c3[k].get("clocks_during_the_same_steps_repeated") or {}
            print("driver configs3 SuBSENSE %-11s %.4f ms/step wall, phase A %.4f ms, fg ratio %.4f; engine clock %s MHz, board power %s W" % (
                k, c3[k]["ms_per_step_wall"], c3[k]["dominant_kernel_avg_ms"], c3[k]["foreground_ratio"], (clk.get("engine_clock_MHz") or {}).get("median"), (clk.get("board_power_W") or {}).get("median")))
        return
    if args.only == "subsense8both":  # young and aged model in one process (A/B scripts)
        run_subsense(8)
        run_subsense(8, warm=300)
        return
    if args.only == "subsense8x2":  # the 8 streams as two / four ranges on their own HIP streams
        run_subsense(8)
        run_subsense(8, groups=2)
        run_subsense(8, groups=4)
        run_subsense(8, kind="smooth", groups=2)
        return
    if args.only == "subsense8agedx2":  # aged model: phase B (sample writes, HBM-bound) of one range beside phase A (VALU-bound) of the other
        run_subsense(8, warm=300)
        run_subsense(8, warm=300, groups=2)
        run_subsense(8, warm=300, groups=4)
        run_subsense(8, warm=300, groups=8)
        return
    if args.only == "subsense8aged1":  # one leg, for counter passes
        run_subsense(8, warm=300, steps=10)
        return
    if args.only == "subsense8aged":  # the model after 300 frames: update rates have settled, far fewer sample writes per frame
        run_subsense(8, warm=300)
        run_subsense(8, kind="smooth", warm=300)
        return
    run(capi.WMV, "WeightedMovingVarianceBGS", 2160, 3840, S, 10)
    run(capi.ABL, "AdaptiveBackgroundLearning", 2160, 3840, S, 10, borrow=False)
    run(capi.WMM, "WeightedMovingMeanBGS (+bg)", 2160, 3840, S, 13, want_bg=True)
    run(capi.FRAME_DIFF, "FrameDifferenceBGS", 2160, 3840, S, 7)
    run(capi.STATIC_FRAME_DIFF, "StaticFrameDifferenceBGS", 2160, 3840, S, 7, borrow=False)
    run(capi.SIGMA_DELTA, "SigmaDeltaBGS", 2160, 3840, S, 16, borrow=False)
    run(capi.ASBL, "AdaptiveSelectiveBackgroundLearning", 2160, 3840, S, 6, borrow=False)
    run(capi.MOG1, "MixtureOfGaussianV1BGS", 1080, 1920, 16, 324, borrow=False)
    pg = capi.default_params(capi.GMG)
    pg.gmg_init_frames = 4  # so the timed frames are normal-operation frames
    run(capi.GMG, "GMG (data-dependent traffic)", 1080, 1920, 8, 16, borrow=False, cpu_frames=8, cpu_warm=5, params=pg)
    run_subsense(2)
    run_subsense(2, kind="smooth")
    run_lbsp()

if __name__ == "__main__":
    main()
