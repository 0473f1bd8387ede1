"""The h3 weight layout on the host (no GPU): `make -C distilcodec_nabeel_amd/csrc w3check` builds
tests/host/w3_layout_check.cpp, a plain C++ program that includes csrc/dcx_w3_layout.h, the header
h2_pack writes through and the kernels take their source offsets from.  It asserts that w3_offset is
a bijection onto [0, phases * taps * Cin * Cout * 2) and that, for every tile origin, DMA instruction
and lane, the offset a kernel computes is that of the element its LDS image expects there
(conv_gemm_x3dq at BN = 128 / 256, conv_gemm_x3dw at BN = 256 / 128, the pair kernels' ring and
per-wave loads at C = 64 / 32).  Run once as built and once under ASan + UBSan."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distilcodec_nabeel_amd", "csrc")


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    r = subprocess.run(["make", "-C", CSRC, "w3check", f"W3CHECK_BIN={exe}", f"W3CHECK_FLAGS={flags}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(exe), "build failed:\n" + (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "w3 layout ok: 7 shapes (5 wide, 2 pair)" in out, out[-4000:]
    return out


def test_w3_layout(tmp_path):
    _build_and_run(tmp_path, "w3_layout_check", "")


def test_w3_layout_under_sanitizers(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    san = "-fsanitize=address,undefined -fno-sanitize-recover=all"
    r = subprocess.run(["g++", *san.split(), str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        pytest.skip("g++ cannot link ASan/UBSan programs on this machine")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = _build_and_run(tmp_path, "w3_layout_check_san", san, env)
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
