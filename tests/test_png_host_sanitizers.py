"""The device PNG encoder's per-segment routine under AddressSanitizer and UBSan (CPU).

tests/host/png_harness.cpp is a program of its own: it includes png_deflate.hpp, is compiled
here with g++ and the scene harness's sanitizer flags, linked with zlib and run as a child
process. It drives rtpng::deflate_segment over a few thousand segments from a fixed seed and
inflates every result with raw zlib (see its head comment). The run must be clean, and both
code-length limiters must have been needed by some segment - else the run says nothing about
them. Nothing is loaded into Python and nothing is preloaded."""
import os
import re
import shutil
import subprocess
from pathlib import Path

from test_host_sanitizers import CSRC, FLAGS, ROOT


def test_png_harness_runs_clean_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the sanitizer harness"
    exe = tmp_path / "png_harness"
    cmd = [gxx, *FLAGS, "-Wall", f"-I{CSRC}", str(ROOT / "tests" / "host" / "png_harness.cpp"), "-lz", "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]   # a sanitizer runtime that does not link fails here

    env = {**os.environ, "UBSAN_OPTIONS": "print_stacktrace=1"}
    run = subprocess.run([str(exe), "5000"], capture_output=True, text=True, env=env, timeout=120)
    print(run.stdout)
    report = run.stderr[-6000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, report
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], report)
    assert run.stdout.strip().endswith("ok")
    m = re.search(r"segments: (\d+), stored: (\d+), ll-limited: (\d+), cl-limited: (\d+)", run.stdout)
    segments, stored, ll, cl = map(int, m.groups())
    assert segments > 5000 and 0 < stored < segments
    assert ll > 0 and cl > 0
