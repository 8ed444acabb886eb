"""Receiver seams (include/adsb_hip.h, "Receiver seams") without a GPU: the declarations in the header, the ctypes
binding, the Rust shim and context.py; the null-handle returns through the loaded library; the header's "Not offered"
sentence still in place with the new section behind it; the support module's expectation on its own catalogue; and the
host code of the mode -- the previous-buffer map and the record merge -- under the address and undefined-behaviour
sanitizers in a stand-alone program (tests/seam_merge_san.cpp)."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path


ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dump1090_rs_amd" / "csrc"

DECLS = ("int adsb_set_receiver_carry(adsb_ctx *ctx, int enabled);",
         "int adsb_get_receiver_carry(const adsb_ctx *ctx);",
         "int adsb_receiver_carry_reset(adsb_ctx *ctx, uint32_t receiver);",
         "int adsb_selftest_rx_seam_tune(adsb_ctx *ctx, uint32_t list_cap);",
         "int adsb_selftest_rx_seam_counters(const adsb_ctx *ctx, uint64_t *out4);")
NAMES = ("adsb_set_receiver_carry", "adsb_get_receiver_carry", "adsb_receiver_carry_reset", "adsb_selftest_rx_seam_tune",
         "adsb_selftest_rx_seam_counters")


def test_the_new_entry_points_are_declared_everywhere():
    header = (ROOT / "include" / "adsb_hip.h").read_text()
    lib_py = (ROOT / "dump1090_rs_amd" / "_lib.py").read_text()
    rust = (ROOT / "integration" / "rust" / "src" / "hip_ffi.rs").read_text()
    context_py = (ROOT / "dump1090_rs_amd" / "context.py").read_text()
    build_py = (ROOT / "dump1090_rs_amd" / "build.py").read_text()
    for decl in DECLS:
        assert decl in header, decl
    assert "#define ADSB_RX_ALL 0xFFFFFFFFu" in header
    for name in NAMES:
        assert f"L.{name}.argtypes" in lib_py, name
        assert f"pub fn {name}(" in rust, name
    for method in ("def set_receiver_carry", "def get_receiver_carry", "def receiver_carry_reset", "def selftest_rx_seam_tune",
                   "def selftest_rx_seam_counters"):
        assert method in context_py, method
    assert '"adsb_seam.hip"' in build_py and '"adsb_seam.cpp"' in build_py


def test_the_not_offered_sentence_stays_and_the_new_section_follows_it():
    header = (ROOT / "include" / "adsb_hip.h").read_text()
    at = header.index("Not offered: carry-over with receivers")
    end = header.index("*/", at)
    sentence = header[at:end]
    for item in ("carry-over with receivers", "valid lengths per", "adsb_multi / the shard calls", "adsb_feed"):
        assert item in sentence, item
    section = header.index("Receiver seams -- carry-over with receivers on")
    assert section > end and section < header.index("Decimation -- IQ sampled at an integer multiple")
    assert header.index("Many receivers, one pass") < at
    body = header[section:header.index("#define ADSB_RX_ALL")]
    # the section says that it is the way to carry-over with receivers, and names what it leaves out
    assert "the way to get carry-over with many receivers" in body
    for item in ("valid lengths per buffer", "scored on the device", "adsb_multi", "adsb_feed"):
        assert item in body[body.index("Not part of this mode"):], item
    for decl in DECLS:
        assert header.index(decl) > section


def test_null_handles_through_the_loaded_library(hip_lib):
    from dump1090_rs_amd import _lib
    L = _lib.lib()
    out4 = (C.c_uint64 * 4)()
    assert L.adsb_set_receiver_carry(None, 1) == _lib.ADSB_ERR_INVALID and L.adsb_set_receiver_carry(None, 0) == _lib.ADSB_ERR_INVALID
    assert L.adsb_get_receiver_carry(None) == _lib.ADSB_ERR_INVALID
    assert L.adsb_receiver_carry_reset(None, 0) == _lib.ADSB_ERR_INVALID
    assert L.adsb_receiver_carry_reset(None, 0xFFFFFFFF) == _lib.ADSB_ERR_INVALID
    assert L.adsb_selftest_rx_seam_tune(None, 4) == _lib.ADSB_ERR_INVALID
    assert L.adsb_selftest_rx_seam_counters(None, out4) == _lib.ADSB_ERR_INVALID


def test_the_expectation_on_the_catalogue(oracle_mod):
    """(A check of the expectation model itself: it runs no code of the library and passes without the feature.)
    The support module against the oracle alone: with carry every straddling and inside frame is found in the seam of
    the buffer that follows it, without carry none is; the frame behind a full-scale last sample is found at j = 325 only
    without carry.  Receivers are independent: a receiver's list does not depend on who else is in the call."""
    from tests import seam_support as S
    streams, planted = S.catalogue(3, 4)
    m = S.round_robin(3, 4)
    iq = S.interleave(streams, m)
    (want,), model = S.expect_calls(3, [(iq, m)])
    (without,), _ = S.expect_calls(3, [(iq, m)], carry=False)
    S.assert_seams_matter(want, without, [f for kind in ("straddle", "inside") for _, f in planted[kind]])
    for kind in ("straddle", "inside"):
        for r, f in planted[kind]:
            assert all(j < S.LEAD and int(m[chunk]) == r for chunk, j, _ in S.found(want, f))
    for _, f in planted["edge"]:
        assert not S.found(want, f) and [j for _, j, _ in S.found(without, f)] == [S.LEAD - 1]
    assert any(model.table(r) for r in range(3))
    # one receiver alone, buffer by buffer
    (alone,), _ = S.expect_calls(1, [(streams[1], [0] * 4)])
    assert [k[1:] for k in alone] == [k[1:] for k in want if int(m[k[0]]) == 1]
    # a reset in front of a call: that receiver's next buffer is a first buffer
    calls = [(iq[:6 * S.CHUNK], m[:6]), (iq[6 * S.CHUNK:], m[6:])]
    plain, _ = S.expect_calls(3, calls)
    reset, _ = S.expect_calls(3, calls, before={1: [("reset", 0)]})
    changed = set(plain[1]) ^ set(reset[1])
    assert plain[0] == reset[0] and changed and all(int(calls[1][1][k[0]]) == 0 and k[1] < S.LEAD for k in changed)


def test_the_host_code_under_address_and_ub_sanitizers():
    """tests/seam_merge_san.cpp, a program of its own (nothing loaded into python)."""
    lib = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    assert lib and Path(lib).exists() and shutil.which("g++") is not None, "g++ and libasan.so are what this test runs on"
    exe = ROOT / "tests" / "seam_merge_asan"
    src = [ROOT / "tests" / "seam_merge_san.cpp", CSRC / "adsb_replay_host.cpp"]
    hdrs = [CSRC / n for n in ("adsb_replay_host.h", "adsb_record.h", "mode_s_host.hpp")] + [ROOT / "include" / "adsb_hip.h"]
    if not exe.exists() or exe.stat().st_mtime < max(p.stat().st_mtime for p in [*src, *hdrs]):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-pthread", *map(str, src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=600,
                       env=dict(__import__("os").environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and "seam merge ok: 400 rounds" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
