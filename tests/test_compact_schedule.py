"""The batch schedule of ldp_restrict_variants()'s in-place compaction (csrc/ldp_compact_schedule.h): the stand-alone checker
tests/sanitize/compact_schedule_check.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer and run on the CPU.  No GPU, nothing
loaded into this process."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_never_reads_an_overwritten_row(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "compact_schedule_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           os.path.join(REPO, "tests", "sanitize", "compact_schedule_check.cpp"), "-o", exe])
    r = subprocess.run([exe, "4000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-400:], r.stderr[-1500:])
    assert "clean" in r.stdout
