"""epilogue_form's lane map on the host (no GPU): `make -C distilcodec_nabeel_amd/csrc epicheck` builds
tests/host/epi_lines_check.cpp, a plain C++ program that includes csrc/dcx_epi_lines.h, the header the
epilogue takes its channel, row, LDS and h2 offsets from.  For the 256 x 256 tiles (passes of 128 and 64
rows) and the 384 x 128 tiles, every pass and row index, tile columns 0 and BN and out_mul 1 ... 3 it
asserts that the map covers each element of a pass exactly once, that the 64 lanes of every global
instruction cover whole 128-byte lines only (fp32 and h2), that the lane pair of an h2 unit holds its two
halves, and that the 16 LDS reads of every 16-lane group fall on 16 distinct bank quads.  Run once as
built and once under ASan + UBSan, as its own executable."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distilcodec_nabeel_amd", "csrc")


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    r = subprocess.run(["make", "-C", CSRC, "epicheck", f"EPICHECK_BIN={exe}", f"EPICHECK_FLAGS={flags}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(exe), "build failed:\n" + (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "epi lines ok: 3 forms" in out, out[-4000:]
    return out


def test_epi_lines(tmp_path):
    _build_and_run(tmp_path, "epi_lines_check", "")


def test_epi_lines_under_sanitizers(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    san = "-fsanitize=address,undefined -fno-sanitize-recover=all"
    r = subprocess.run(["g++", *san.split(), str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        pytest.skip("g++ cannot link ASan/UBSan programs on this machine")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = _build_and_run(tmp_path, "epi_lines_check_san", san, env)
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
