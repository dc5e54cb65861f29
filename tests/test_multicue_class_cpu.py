"""SJN_MultiCueBGS as a class, without a GPU: header, binding and library agreement for the per-stream lifetime, the
range call and the host-memory call; the syntax checks of both sides of the host layer (what its classes write and print is pinned by
tests/test_host_classes_cpu.py); and bgs_demo through FrameProcessor::enableMultiCueBGS up to the one exception a machine without a
device ends in.  There is still no algorithm id: bgs_abi_version() and ALGO_LAST stay where they were."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tracking_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgs_hip.h")
HOST = os.path.join(ROOT, "tracking_amd", "host")


def test_header_binding_and_library_agree():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = C.CDLL(capi.LIB_PATH)
    bound = {n: a for n, _, a in capi.SYMBOLS}
    for n, nargs in (("bgs_multicue_process_range_device", 8), ("bgs_multicue_reset_stream", 2), ("bgs_multicue_process", 9)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, h)
        assert m and len(m.group(1).split(",")) == nargs == len(bound[n]), n
        assert hasattr(lib, n), n
    assert capi.lib().bgs_abi_version() == 1 and capi.ALGO_LAST == 37  # the class has no algorithm id


def test_frame_processor_compiles_without_warnings():
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(HOST, "FrameProcessor.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_reference_side_adapters_compile_with_the_class(tmp_path):
    tu = tmp_path / "adapters_multicue.cpp"
    tu.write_text('#include "HipBGS.h"\n#include "HipFGDetector.h"\nIBGS* a() { return new hipbgs::SJN_MultiCueBGS; }\n')
    r = subprocess.run(["g++", "-std=gnu++0x", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_opencv"), "-I" + os.path.join(ROOT, "include"),
                        "-I" + HOST, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_frame_processor_builds_the_class_and_writes_the_reference_xml(tmp_path):
    """Without a GPU the first frame ends in the one exception of the host layer; by then saveConfig() has written the reference's one
    key.  With a GPU the run succeeds."""
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    demo = os.path.join(ROOT, "tracking_amd", "lib", "bgs_demo")
    wd = str(tmp_path)
    os.makedirs(os.path.join(wd, "config"))
    raw = os.path.join(wd, "frames.raw")
    np.zeros((2, 8, 8, 3), np.uint8).tofile(raw)
    with open(os.path.join(wd, "config", "FrameProcessor.xml"), "w") as f:
        f.write('<?xml version="1.0"?>\n<opencv_storage>\n<enableFrameDifferenceBGS>0</enableFrameDifferenceBGS>\n<enableMultiCueBGS>1</enableMultiCueBGS>\n</opencv_storage>\n')
    r = subprocess.run([demo, raw, "8", "8", "2", os.path.join(wd, "out")], cwd=wd, capture_output=True, text=True)
    assert "MultiCueBGS()" not in r.stdout, r.stdout  # no banner
    assert r.returncode == 0 or (r.stdout.count("std::exception:") == 1 and "no HIP device" in r.stdout), r.stdout + r.stderr
    xml = open(os.path.join(wd, "config", "MultiCueBGS.xml")).read()
    assert xml == '<?xml version="1.0"?>\n<opencv_storage>\n<showOutput>1</showOutput>\n</opencv_storage>\n'
    assert "<enableMultiCueBGS>1</enableMultiCueBGS>" in open(os.path.join(wd, "config", "FrameProcessor.xml")).read()
