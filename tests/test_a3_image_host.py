"""conv_gemm_x3dw's activation image on the host (no GPU): `make -C distilcodec_nabeel_amd/csrc a3check`
builds tests/host/a3_image_check.cpp, a plain C++ program that includes csrc/dcx_a3_layout.h, the header
x3dw_tile takes its LDS-DMA source offsets and its fragment addresses from.  For every tile form (image
rows 320 / 256 / 448 / 384), row pitch, chunk and tap offset 0 ... 64 it asserts that the DMA
instructions' lanes map one-to-one onto the image, that each lane fetches the (row, piece) its image
byte is read as, that an instruction touches exactly 8 128-byte lines, and that the 16 addresses of
every ds_read_b128 lane group fall on 16 distinct 16-byte slots.  Run once as built and once under
ASan + UBSan."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distilcodec_nabeel_amd", "csrc")


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    r = subprocess.run(["make", "-C", CSRC, "a3check", f"A3CHECK_BIN={exe}", f"A3CHECK_FLAGS={flags}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(exe), "build failed:\n" + (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "a3 image ok: 4 forms" in out, out[-4000:]
    return out


def test_a3_image(tmp_path):
    _build_and_run(tmp_path, "a3_image_check", "")


def test_a3_image_under_sanitizers(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    san = "-fsanitize=address,undefined -fno-sanitize-recover=all"
    r = subprocess.run(["g++", *san.split(), str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        pytest.skip("g++ cannot link ASan/UBSan programs on this machine")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = _build_and_run(tmp_path, "a3_image_check_san", san, env)
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
