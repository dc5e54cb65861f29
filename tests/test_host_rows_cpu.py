"""The row functions of the host path (tracking_amd/csrc/host_rows.h: the band split, packing through the flip / ROI row map, unpacking,
unpacking to three channels) against naive loops, under AddressSanitizer and UBSan.  The checks are tests/host_rows_main.cpp, a program
of its own: nothing of Python runs in the sanitized process."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_row_functions_sanitized(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "the row test needs g++"
    exe = str(tmp_path / "host_rows")
    # -static-lib*: the sanitizer runtimes are linked into the program, which keeps them first in its link order without touching the
    # environment of the process
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(HERE, "host_rows_main.cpp")], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 checks failed"), r.stdout[-4000:]
