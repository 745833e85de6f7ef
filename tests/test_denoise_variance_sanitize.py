"""tests/c/denoise_variance_ref.c's stand-alone program (-DDENOISE_VARIANCE_REF_MAIN: the edge sizes, every
guide subset, the luminance term and the spatial estimate on and off, separate and in-place outputs)
built with the address and undefined sanitizers and run once. CPU only; nothing loaded into Python is
involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "denoise_variance_ref.c")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    for name in ("libasan.so", "libubsan.so"):
        r = subprocess.run([gcc, f"-print-file-name={name}"], capture_output=True, text=True)
        if not os.path.isabs(r.stdout.strip()):
            pytest.skip(f"the toolchain has no {name}")
    out = str(tmp_path_factory.mktemp("denoise_variance_ref") / "denoise_variance_ref")
    cmd = [gcc, "-std=c11", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DDENOISE_VARIANCE_REF_MAIN", SRC, "-lm", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_reference_is_sanitizer_clean(exe):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1].startswith("denoise_variance_ref ok"), r.stdout[-400:]
