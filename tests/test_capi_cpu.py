"""CPU-side checks of the drop-in boundary: the library loads, exports every symbol include/bgs_hip.h declares,
the ctypes struct mirrors the C struct, and — on a box without a GPU — compute entry points fail loudly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tracking_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgs_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bgs_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported():
    names = declared_functions()
    assert len(names) >= 15
    lib = C.CDLL(capi.LIB_PATH)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert sorted(n for n, _, _ in capi.SYMBOLS) == names, "capi.SYMBOLS must bind exactly what the header declares"


def test_params_struct_matches_c(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(bgs_params), '
                   'offsetof(bgs_params, alpha), offsetof(bgs_params, mog2_var_threshold), offsetof(bgs_params, sd_max_var));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, a, b, c = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(capi.BgsParams)
    assert a == capi.BgsParams.alpha.offset and b == capi.BgsParams.mog2_var_threshold.offset and c == capi.BgsParams.sd_max_var.offset


def test_abi_version_and_defaults():
    assert capi.lib().bgs_abi_version() == 1
    p = capi.default_params(capi.MOG2)
    assert (p.threshold, p.enable_threshold, p.alpha) == (15, 1, 0.05)  # MixtureOfGaussianV2BGS.cpp:90-97
    assert (p.mog2_nmixtures, p.mog2_var_threshold, p.mog2_var_threshold_gen) == (5, 16.0, 9.0)
    assert capi.default_params(capi.ASBL).threshold == 25  # AdaptiveSelectiveBackgroundLearning.cpp:127
    assert capi.default_params(capi.ASBL).learning_frames == 90


def test_defaults_agree_with_oracle():
    from oracle import pyoracle
    for algo in range(18):
        a = capi.default_params(algo)
        b = capi.BgsParams()
        b.struct_size = C.sizeof(capi.BgsParams)
        assert pyoracle.lib().orc_default_params(algo, C.byref(b)) == 0
        assert bytes(a) == bytes(b), algo


def test_bad_arguments_are_reported():
    h = C.c_void_p()
    assert capi.lib().bgs_create(99, None, 0, 1, C.byref(h)) == capi.ERR_INVALID
    assert b"unknown algorithm" in capi.lib().bgs_last_error()
    assert capi.lib().bgs_create(capi.MOG2, None, 0, 0, C.byref(h)) == capi.ERR_INVALID
    p = capi.default_params(capi.MOG2)
    p.struct_size = 8
    assert capi.lib().bgs_create(capi.MOG2, C.byref(p), 0, 1, C.byref(h)) == capi.ERR_INVALID
    p = capi.default_params(capi.MOG2)
    p.mog2_nmixtures = 3
    assert capi.lib().bgs_create(capi.MOG2, C.byref(p), 0, 1, C.byref(h)) == capi.ERR_UNSUPPORTED


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    rc = capi.lib().bgs_create(capi.MOG2, None, 0, 1, C.byref(h))
    assert rc == capi.ERR_HIP and not h.value
    assert b"no CPU path" in capi.lib().bgs_last_error()


def test_product_never_touches_the_oracle():
    """oracle/ is test infrastructure: nothing under tracking_amd/ or include/ may reference it."""
    bad = []
    for base in ("tracking_amd", "include"):
        for dp, _, fns in os.walk(os.path.join(ROOT, base)):
            if os.sep + "lib" in dp:
                continue
            for fn in fns:
                if fn.endswith((".py", ".h", ".hip", ".cpp", ".c", "Makefile")):
                    t = open(os.path.join(dp, fn), errors="replace").read()
                    if "oracle" in t.replace("no oracle", ""):
                        bad.append(os.path.join(dp, fn))
    assert not bad, bad


def test_reference_side_adapters_compile(tmp_path):
    """tracking_amd/host/HipBGS.h and HipFGDetector.h (what a maintainer adds to the reference tree: cv::Mat, CvFileStorage, CvFGDetector,
    CvBlobSeq) are syntax-checked as -std=gnu++0x - the reference's CMakeLists.txt:5 - against the declaration-only OpenCV mock in
    tests/mock_opencv.  Nothing is linked or run: OpenCV itself is absent from this image."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tu = tmp_path / "adapters.cpp"
    tu.write_text('#include "HipBGS.h"\n#include "HipFGDetector.h"\n'
                  'IBGS* make(int i) { return i ? (IBGS*)new hipbgs::MixtureOfGaussianV2BGS : (IBGS*)new hipbgs::SuBSENSEBGS(); }\n'
                  'CvFGDetector* make_fg() { return new HipFGDetector(36); }\n'
                  'int blobs(HipFGDetector* d, CvBlobSeq* s) { return d->GetBlobs(s) + d->GetBlobs(s, 4, false); }\n')
    r = subprocess.run(["g++", "-std=gnu++0x", "-fsyntax-only", "-Wall", "-I" + os.path.join(root, "tests", "mock_opencv"), "-I" + os.path.join(root, "include"),
                        "-I" + os.path.join(root, "tracking_amd", "host"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_blob_conversions_on_known_shapes(tmp_path):
    """tracking_amd/host/blob_convert.h: a filled w x h rectangle at (x0, y0) gives, from its box, centre (x0 + w/2, y0 + h/2) and size
    (w, h); from its moments, the centroid (x0 + (w-1)/2, y0 + (h-1)/2) and 4 sigma of a discrete uniform: 4 sqrt((w^2-1)/12)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include <cstdio>
#include "blob.h"
using namespace bgs_hip;
int main() {
  const int x0 = 10, y0 = 20, w = 7, h = 4;
  bgs_box b = {x0, y0, w, h, w * h, y0 * 100 + x0};
  bgs_moments m = {0, 0, 0, 0};
  for (int y = y0; y < y0 + h; ++y) for (int x = x0; x < x0 + w; ++x) m.sx += x, m.sy += y, m.sxx += x * x, m.syy += y * y;
  CvBlob a = cvBlob(0, 0, 0, 0), c = cvBlob(0, 0, 0, 0);
  bgs_hip_convert::blob_from_box(b, a);
  bgs_hip_convert::blob_from_moments(b, m, c);
  std::printf("%.6f %.6f %.6f %.6f | %.6f %.6f %.6f %.6f\n", a.x, a.y, a.w, a.h, c.x, c.y, c.w, c.h);
  CvBlobSeq s; s.AddBlob(&a); c.ID = 5; s.AddBlob(&c);
  std::printf("%d %d %d\n", s.GetBlobNum(), s.GetBlobByID(5) == s.GetBlob(1), s.GetBlob(2) == 0);
  s.DelBlob(0); std::printf("%d %d\n", s.GetBlobNum(), s.GetBlob(0)->ID);
  return 0;
}''')
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++14", "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "tracking_amd", "host"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    box, mom = [[float(v) for v in part.split()] for part in out[0].split("|")]
    assert box == [13.5, 22.0, 7.0, 4.0]
    want = [10 + 3.0, 20 + 1.5, 4 * np.sqrt((49 - 1) / 12.0), 4 * np.sqrt((16 - 1) / 12.0)]
    assert np.allclose(mom, want, atol=1e-5), (mom, want)
    assert out[1].split() == ["2", "1", "1"] and out[2].split() == ["1", "5"]


def test_ingest_and_blob_structs_match_c(tmp_path):
    """bgs_ingest (ctypes mirror capi.BgsIngest), bgs_box and bgs_moments (numpy int32 x 6 / int64 x 4 rows in the bindings) have the
    layout the C compiler gives them; bgs_ingest_default / bgs_ingest_size / bgs_ingest_workspace answer without a GPU."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(bgs_ingest), offsetof(bgs_ingest, roi_x0), '
                   'offsetof(bgs_ingest, gaussian_blur), sizeof(bgs_box), sizeof(bgs_moments));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, roi, blur, box, mom = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(capi.BgsIngest) and roi == capi.BgsIngest.roi_x0.offset and blur == capi.BgsIngest.gaussian_blur.offset
    assert box == 6 * 4 and mom == 4 * 8
    c = capi.default_ingest()
    assert (c.struct_size, c.resize_percent, c.flip, c.equalize_hist, c.gaussian_blur) == (size, 100, 0, 0, 0)
    r, k = C.c_int(0), C.c_int(0)
    assert capi.lib().bgs_ingest_size(C.byref(c), 1080, 1920, C.byref(r), C.byref(k)) == 0 and (r.value, k.value) == (1080, 1920)
    c2 = capi.default_ingest(resize_percent=50, roi_x0=10, roi_y0=20, roi_x1=110, roi_y1=70, gaussian_blur=1)
    assert capi.lib().bgs_ingest_size(C.byref(c2), 1080, 1920, C.byref(r), C.byref(k)) == 0 and (r.value, k.value) == (50, 100)
    assert capi.lib().bgs_ingest_workspace(C.byref(c2), 4, 1080, 1920, 3) >= 4 * 50 * 100 * 3
    assert capi.lib().bgs_ingest_workspace(C.byref(c), 4, 1080, 1920, 3) == 0
    bad = capi.default_ingest(roi_x0=10, roi_y0=20, roi_x1=5000, roi_y1=70)
    assert capi.lib().bgs_ingest_size(C.byref(bad), 1080, 1920, C.byref(r), C.byref(k)) == capi.ERR_INVALID
