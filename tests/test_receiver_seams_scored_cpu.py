"""Receiver seams scored on the device (include/adsb_hip.h, "Receiver seams, scored on the device") without a GPU: the
declarations in the header, the ctypes binding and context.py; the null-handle returns through the loaded library; the new
unit in the build's list; and the index arithmetic and classification the device-side merge is written with
(csrc/adsb_seam_score_dev.h) under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/seam_score_index_san.cpp), against the host's own merge (merge_seam_records)."""
import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dump1090_rs_amd" / "csrc"

DECLS = ("int adsb_set_receiver_carry_scoring(adsb_ctx *ctx, int enabled);",
         "int adsb_get_receiver_carry_scoring(const adsb_ctx *ctx);",
         "int adsb_selftest_rx_seam_score_counters(const adsb_ctx *ctx, uint64_t *out4);")


def test_the_header_declares_the_mode_and_keeps_the_single_modes_refusal():
    text = (ROOT / "include" / "adsb_hip.h").read_text()
    for d in DECLS:
        assert d in text, d
    assert "Receiver seams, scored on the device" in text
    # the two single setters still refuse each other, in the words they always had
    assert "and while adsb_set_receiver_scoring is on" in text and "seam trials are" in text


def test_the_binding_and_the_null_handle_returns(hip_lib):
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd.context import Context
    L = _lib.lib()
    assert L.adsb_set_receiver_carry_scoring(None, 1) == _lib.ADSB_ERR_INVALID
    assert L.adsb_get_receiver_carry_scoring(None) == _lib.ADSB_ERR_INVALID
    out = (C.c_uint64 * 4)()
    assert L.adsb_selftest_rx_seam_score_counters(None, out) == _lib.ADSB_ERR_INVALID
    assert L.adsb_selftest_reservations(None) == 0
    for name in ("set_receiver_carry_scoring", "get_receiver_carry_scoring", "selftest_rx_seam_score_counters"):
        assert callable(getattr(Context, name)), name


def test_the_unit_is_built_and_declared():
    build = (ROOT / "dump1090_rs_amd" / "build.py").read_text()
    assert '"adsb_seam_score.hip"' in build and '"adsb_seam_score_dev.h"' in build
    assert "launch_seam_merge" in (CSRC / "adsb_device.h").read_text()


def test_the_index_header_under_address_and_ub_sanitizers():
    """tests/seam_score_index_san.cpp, a program of its own (nothing loaded into python)."""
    lib = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    assert lib and Path(lib).exists() and shutil.which("g++") is not None, "g++ and libasan.so are what this test runs on"
    exe = ROOT / "tests" / "seam_score_index_asan"
    src = [ROOT / "tests" / "seam_score_index_san.cpp", CSRC / "adsb_replay_host.cpp"]
    hdrs = [CSRC / n for n in ("adsb_seam_score_dev.h", "adsb_replay_host.h", "adsb_record.h", "mode_s_host.hpp")] + [ROOT / "include" / "adsb_hip.h"]
    if not exe.exists() or exe.stat().st_mtime < max(p.stat().st_mtime for p in [*src, *hdrs]):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-pthread", *map(str, src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "600"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and "seam score index ok: 600 rounds" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
