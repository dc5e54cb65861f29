"""The host layer (tracking_amd/host) run, not read: tests/host_classes_main.cpp constructs each of the 34 IBGS classes, FrameProcessor
and USTC_BGS(-1 .. 38) with no device visible; the ./config/*.xml files it leaves and its stdout are compared byte for byte with
tests/golden/host_config/.  Every class writes its XML before it asks for an engine, so this needs no GPU; where there is one, the
child processes do not see it.  The fixtures are what the program printed and wrote when they were recorded:
    python tests/test_host_classes_cpu.py --record      (after `make -C tracking_amd/host`)
rewrites them from the current host layer; a change of this layer that is meant to keep its behaviour leaves them as they are.

    defaults/       written with no ./config file present (34 classes, and FrameProcessor.xml by FrameProcessor's constructor)
    nondefault/     input: every key of every class at a value that is not its default, reals that are no float, the preloadModel string,
                    MultiLayerBGS with loadDefaultParams 0; FrameProcessor.xml with every enable flag set and a tictoc name
    rewritten/      what the first process() call (FrameProcessor: the constructor) makes of nondefault/
    ldp1/           MultiLayerBGS.in.xml = nondefault/ with loadDefaultParams 1, MultiLayerBGS.out.xml = what the hard-coded block leaves
    stdout.txt      the runs' stdout: banners in construction and teardown order, exception texts, the type table
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tracking_amd", "host")
LIB = os.path.join(ROOT, "tracking_amd", "lib")
GOLD = os.path.join(ROOT, "tests", "golden", "host_config")

# the order of tests/host_classes_main.cpp; SJN_MultiCueBGS keeps its settings in ./config/MultiCueBGS.xml (SJN_MultiCueBGS.cpp:115-131)
CLASSES = ["FrameDifferenceBGS", "StaticFrameDifferenceBGS", "WeightedMovingMeanBGS", "WeightedMovingVarianceBGS", "AdaptiveBackgroundLearning",
           "AdaptiveSelectiveBackgroundLearning", "MixtureOfGaussianV2BGS", "MixtureOfGaussianV1BGS", "GMG", "SigmaDeltaBGS", "SuBSENSEBGS", "LOBSTERBGS",
           "DPZivkovicAGMMBGS", "DPGrimsonGMMBGS", "DPWrenGABGS", "DPMeanBGS", "DPAdaptiveMedianBGS", "KDE", "DPPratiMediodBGS", "DPTextureBGS",
           "LBSimpleGaussian", "LBFuzzyGaussian", "LBMixtureOfGaussians", "LBAdaptiveSOM", "LBFuzzyAdaptiveSOM", "VuMeter", "FuzzySugenoIntegral",
           "FuzzyChoquetIntegral", "T2FGMM_UM", "T2FGMM_UV", "DPEigenbackgroundBGS", "IndependentMultimodalBGS", "MultiLayerBGS", "SJN_MultiCueBGS"]
XML = [c + ".xml" for c in CLASSES[:-1]] + ["MultiCueBGS.xml"]
SOURCES = [os.path.join(ROOT, "tests", "host_classes_main.cpp"), os.path.join(HOST, "FrameProcessor.cpp")]
FLAGS = ["-std=c++14", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + HOST]
LINK = ["-L" + LIB, "-lbgs_hip", "-Wl,-rpath," + LIB]


def compile_program(exe, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "the host-layer test needs g++"
    assert os.path.exists(os.path.join(LIB, "libbgs_hip.so")), "build() makes tracking_amd/lib/libbgs_hip.so"
    subprocess.run([gxx] + FLAGS + list(extra) + ["-o", exe] + SOURCES + LINK, check=True)
    return exe


def run(exe, wd, *args, **env):
    """One run in wd; no device is visible to it, so every machine sees what a machine without one sees."""
    os.makedirs(os.path.join(wd, "config"), exist_ok=True)
    e = {k: v for k, v in os.environ.items() if k != "BGS_HOST_NO_GROUP"}
    e.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", **env)
    r = subprocess.run([exe] + list(args), cwd=wd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def run_all(exe, base):
    """The six runs.  Returns (stdout text, {fixture path relative to GOLD: path of the file the run left})."""
    wd = {k: os.path.join(base, k) for k in ("defaults", "rewritten", "ldp1", "fp_defaults", "fp_all")}
    out, files = [], {}
    out.append("== classes, no ./config file\n" + run(exe, wd["defaults"], "classes"))
    os.makedirs(os.path.join(wd["rewritten"], "config"))
    for f in XML:
        shutil.copy(os.path.join(GOLD, "nondefault", f), os.path.join(wd["rewritten"], "config", f))
    out.append("== classes, every key at a value that is not its default\n" + run(exe, wd["rewritten"], "classes"))
    os.makedirs(os.path.join(wd["ldp1"], "config"))
    shutil.copy(os.path.join(GOLD, "ldp1", "MultiLayerBGS.in.xml"), os.path.join(wd["ldp1"], "config", "MultiLayerBGS.xml"))
    out.append("== MultiLayerBGS, loadDefaultParams 1\n" + run(exe, wd["ldp1"], "classes", "MultiLayerBGS"))
    out.append("== FrameProcessor, no ./config file\n" + run(exe, wd["fp_defaults"], "fp"))
    os.makedirs(os.path.join(wd["fp_all"], "config"))
    shutil.copy(os.path.join(GOLD, "nondefault", "FrameProcessor.xml"), os.path.join(wd["fp_all"], "config"))
    out.append("== FrameProcessor, every enable flag set, BGS_HOST_NO_GROUP=1\n" + run(exe, wd["fp_all"], "fp", BGS_HOST_NO_GROUP="1"))
    out.append("== USTC_BGS(t), t = -1 .. 38\n" + run(exe, wd["defaults"], "ustc"))
    for f in XML:
        files["defaults/" + f] = os.path.join(wd["defaults"], "config", f)
        files["rewritten/" + f] = os.path.join(wd["rewritten"], "config", f)
    files["ldp1/MultiLayerBGS.out.xml"] = os.path.join(wd["ldp1"], "config", "MultiLayerBGS.xml")
    files["defaults/FrameProcessor.xml"] = os.path.join(wd["fp_defaults"], "config", "FrameProcessor.xml")
    files["rewritten/FrameProcessor.xml"] = os.path.join(wd["fp_all"], "config", "FrameProcessor.xml")
    return "".join(out), files


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    base = str(tmp_path_factory.mktemp("host_classes"))
    return run_all(compile_program(os.path.join(base, "host_classes")), base)


def section(text, title):
    return text.split("== " + title + "\n", 1)[1].split("\n== ", 1)[0] + "\n"


def test_every_xml_file_equals_its_fixture(ran):
    """Key order, key names, value formats, every default (defaults/), every key's way from the file into its member and back, the (float)
    narrowing, the int-typed dp thresholds, the string key (rewritten/), MultiLayerBGS's hard-coded block (ldp1/), FrameProcessor's
    enable keys with their defaults and order: one byte-for-byte comparison per file."""
    _, files = ran
    assert len(files) == 2 * 34 + 3
    for rel, path in sorted(files.items()):
        assert os.path.exists(path), rel + " was not written"
        assert open(path, "rb").read() == open(os.path.join(GOLD, rel), "rb").read(), rel


def test_inputs_really_differ_from_the_defaults():
    """The round trip says nothing for a key whose input value is its default: every value line of nondefault/ differs from defaults/."""
    for f in XML + ["FrameProcessor.xml"]:
        a = open(os.path.join(GOLD, "defaults", f)).read().split("\n")
        b = open(os.path.join(GOLD, "nondefault", f)).read().split("\n")
        assert len(a) == len(b), f
        same = [x for x, y in zip(a, b) if x == y and not x.startswith(("<?xml", "<opencv_storage>", "</opencv_storage>")) and x]
        # the two flags that are on by default stay on: the FrameProcessor run is the one with every enable flag set
        assert same == (["<enablePreProcessor>1</enablePreProcessor>", "<enableFrameDifferenceBGS>1</enableFrameDifferenceBGS>"] if f == "FrameProcessor.xml" else []), (f, same)
    ml = open(os.path.join(GOLD, "nondefault", "MultiLayerBGS.xml")).read()
    assert "<loadDefaultParams>0</loadDefaultParams>" in ml and '<preloadModel>"model.bin"</preloadModel>' in ml
    assert open(os.path.join(GOLD, "ldp1", "MultiLayerBGS.in.xml")).read() == ml.replace("<loadDefaultParams>0<", "<loadDefaultParams>1<")


def test_stdout_equals_its_fixture(ran):
    """Constructor and destructor banners (and the classes that print none), the one exception of a machine without a device with the
    class's name in front, FrameProcessor's construction order and its teardown order (~IndependentMultimodalBGS() before
    ~MultiLayerBGS(): not the reverse of init()), which USTC_BGS types build which class and which are refused with which text."""
    text, _ = ran
    want = open(os.path.join(GOLD, "stdout.txt")).read()
    for title in [l[3:] for l in want.split("\n") if l.startswith("== ")]:
        assert section(text, title) == section(want, title), title
    assert text == want


def test_the_fixture_says_what_the_issue_pins():
    """The facts earlier tests read out of the source text, read out of the recorded run instead (so the byte comparison above asserts them)."""
    want = open(os.path.join(GOLD, "stdout.txt")).read()
    table = {}
    for block in section(want, "USTC_BGS(t), t = -1 .. 38").split("-- type ")[1:]:
        lines = block.strip().split("\n")
        table[int(lines[0])] = lines[1:]
    assert sorted(table) == list(range(-1, 39))
    refused = [t for t in table if len(table[t]) == 1 and table[t][0] == "std::exception:USTC_BGS: type %d is outside the package_bgs hot path built here" % t]
    assert refused == [15, 19, 20, 23, 24, 30, 33, 34]
    assert table[-1] == table[38] == ["std::exception:USTC_BGS: type must be 0..37"]
    built = {t: table[t][0][:-2] for t in table if "built" in table[t]}
    assert len(built) == 30 and all(table[t][0] == built[t] + "()" and table[t][1] == "built" for t in built)
    assert [built[t] for t in (17, 18, 21, 22, 25, 26, 27, 28, 29, 31, 32, 14, 16)] == ["T2FGMM_UM", "T2FGMM_UV", "FuzzySugenoIntegral", "FuzzyChoquetIntegral", "LBSimpleGaussian",
        "LBFuzzyGaussian", "LBMixtureOfGaussians", "LBAdaptiveSOM", "LBFuzzyAdaptiveSOM", "VuMeter", "KDE", "DPPratiMediodBGS", "DPTextureBGS"]
    fp = section(want, "FrameProcessor, every enable flag set, BGS_HOST_NO_GROUP=1").split("\n")
    assert fp.index("~IndependentMultimodalBGS()") + 1 == fp.index("~MultiLayerBGS()") and fp.index("IndependentMultimodalBGS()") + 1 == fp.index("MultiLayerBGS()")
    assert "groupedClasses 0" in fp and not [l for l in fp if "MultiCue" in l]  # SJN_MultiCueBGS prints no banner
    # the reference-side detector cannot be run here: its type table is text, and it is held to the table the run recorded
    det = open(os.path.join(HOST, "HipFGDetector.h")).read()
    for t in range(38):
        if t in built:
            assert det.count("bgs = new hipbgs::%s" % built[t]) == 1 and ("(i == %d) bgs = new hipbgs::%s" % (t, built[t]) in det or "case %d: bgs = new hipbgs::%s;" % (t, built[t]) in det), t
        else:
            assert "i == %d)" % t not in det and "case %d:" % t not in det, t


def test_both_headers_include_the_same_class_files():
    """Text about text: HipBGS.h (cv::Mat, for the reference tree, not runnable here) and bgs_host.h (what the runs above ran) include the
    same class files in the same order, each once, and every .inc of the directory is among them."""
    import re
    lists = [re.findall(r'^#include "(\w+\.inc)"', open(os.path.join(HOST, f)).read(), re.M) for f in ("HipBGS.h", "bgs_host.h")]
    assert lists[0] == lists[1] and len(set(lists[0])) == len(lists[0])
    assert sorted(lists[0]) == sorted(f for f in os.listdir(HOST) if f.endswith(".inc"))


def test_reference_side_adapters_compile_with_all_34_classes(tmp_path):
    """HipBGS.h / HipFGDetector.h as -std=gnu++0x (the reference's CMakeLists.txt:5) against the declaration-only OpenCV mock, every
    hipbgs:: class instantiated: each class exists in that namespace too and its description compiles in the language the reference uses."""
    tu = tmp_path / "adapters_all.cpp"
    tu.write_text('#include "HipBGS.h"\n#include "HipFGDetector.h"\nIBGS* make(int i) {\n'
                  + "".join("  if (i == %d) return new hipbgs::%s;\n" % (k, c) for k, c in enumerate(CLASSES))
                  + "  return 0;\n}\nvoid more(hipbgs::MultiLayerBGS* m, hipbgs::SJN_MultiCueBGS* s, hipbgs::KDE* k) { m->setStatus(hipbgs::MultiLayerBGS::MLBGS_LEARN); s->setDevice(1); k->setDevice(1); }\n"
                  "CvFGDetector* make_fg(int t) { return new HipFGDetector(t); }\nint blobs(HipFGDetector* d, CvBlobSeq* s) { return d->GetBlobs(s) + d->GetBlobs(s, 4, false); }\n")
    r = subprocess.run(["g++", "-std=gnu++0x", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_opencv"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr


def test_the_runs_are_clean_under_asan_and_ubsan(tmp_path, monkeypatch):
    """The same program with -fsanitize=address,undefined (runtimes linked in statically: nothing is preloaded), leak detection on for
    the host layer.  libbgs_hip.so and the HIP runtime under it are not instrumented; where a GPU is installed the runtime's start-up
    keeps 144 bytes in libhsa-runtime64 although the device is hidden, so leaks whose stack runs through those three libraries are
    suppressed - the host layer's own allocations (the program, FrameProcessor.cpp, the headers) are not.  Same runs, same output."""
    exe = compile_program(str(tmp_path / "host_classes_san"), ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    supp = tmp_path / "lsan.supp"
    supp.write_text("leak:libbgs_hip\nleak:libamdhip64\nleak:libhsa-runtime64\n")
    monkeypatch.setenv("LSAN_OPTIONS", "suppressions=%s:print_suppressions=0" % supp)
    text, _ = run_all(exe, str(tmp_path))
    assert text == open(os.path.join(GOLD, "stdout.txt")).read()


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    import tempfile
    with tempfile.TemporaryDirectory() as base:
        text, files = run_all(compile_program(os.path.join(base, "host_classes")), base)
        for rel, path in files.items():
            os.makedirs(os.path.dirname(os.path.join(GOLD, rel)), exist_ok=True)
            shutil.copy(path, os.path.join(GOLD, rel))
        open(os.path.join(GOLD, "stdout.txt"), "w").write(text)
    print("recorded %d files and stdout.txt under %s" % (len(files), GOLD))
