"""The mixer (include/adsb_hip.h, "Frequency shift") without a GPU: its ABI in the header, the library, the Rust shim and
the Python package, the table and the shift arithmetic (host only), the argument checks that need no device, adsb_feed's
usage, and the numpy restatement the GPU tests hold the device to (tests/mix_support.py) checked against itself."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from tests import decim_support as ds
from tests import mix_support as ms
from tests import resamp_support as rs
from tests import test_rust_shim as shim
from tests.conftest import ROOT

HEADER = ROOT / "include" / "adsb_hip.h"
FFI = ROOT / "integration" / "rust" / "src" / "hip_ffi.rs"
NAMES = ("adsb_mix_set_decim", "adsb_mix_set_resamp", "adsb_mix_get_decim", "adsb_mix_get_resamp", "adsb_mix_table",
         "adsb_mix_for_shift")
PATTERN = r"adsb_mix_\w+"


def header_prototypes():
    text = shim.strip_comments(HEADER.read_text())
    out = {}
    for m in re.finditer(r"(?:ADSB_MUST_CHECK|extern)?\s*\b(int|void|uint32_t)\s+(" + PATTERN + r")\s*\(([^)]*)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        params = [shim.c_type_to_rust(re.match(r"^(.*?)(\w+)$", a.strip()).group(1).strip()) for a in args.split(",")]
        out[name] = (params, shim.c_type_to_rust(ret))
    return out


def rust_prototypes():
    text = shim.strip_comments(FFI.read_text())
    out = {}
    for f in re.finditer(r"pub\s+fn\s+(" + PATTERN + r")\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", text, flags=re.S):
        args = " ".join(f.group(2).split())
        params = [" ".join(a.split(":", 1)[1].split()) for a in args.split(",") if a.strip()]
        out[f.group(1)] = (params, " ".join(f.group(3).split()) if f.group(3) else None)
    return out


def test_the_functions_are_declared_exported_and_bound(hip_lib, monkeypatch):
    import dump1090_rs_amd as pkg
    monkeypatch.setitem(shim.BASE, "adsb_decim", "AdsbDecim")
    monkeypatch.setitem(shim.BASE, "adsb_resamp", "AdsbResamp")
    hdr, ffi = header_prototypes(), rust_prototypes()
    assert sorted(hdr) == sorted(NAMES) == sorted(ffi)
    for name in hdr:
        assert hdr[name] == ffi[name], f"{name}: header {hdr[name]} vs hip_ffi.rs {ffi[name]}"
        assert hasattr(hip_lib, name), f"{name} is not exported"
        assert len(getattr(hip_lib, name).argtypes) == len(hdr[name][0]), name
    assert hdr["adsb_mix_set_decim"] == (["*mut AdsbDecim", "*const i16", "u32"], "c_int")
    assert hdr["adsb_mix_get_resamp"] == (["*const AdsbResamp"], "u32")
    assert hdr["adsb_mix_for_shift"] == (["u32", "u32", "i32", "*mut u32", "*mut u32"], "c_int")
    assert "#define ADSB_MIX_MAX_PERIOD 256u" in HEADER.read_text()
    for name in ("mixer_table", "mixer_for_shift"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for cls in (pkg.Decimator, pkg.Resampler):
        assert hasattr(cls, "set_mixer") and isinstance(cls.mixer_period, property)


def test_mix_table_properties(hip_lib):
    from dump1090_rs_amd import _lib, mixer_table
    from dump1090_rs_amd._lib import AdsbError
    # exact rotations at N = 1, 2, 4 -- pinned
    assert mixer_table(0, 1).tolist() == [[16384, 0]]
    assert mixer_table(1, 2).tolist() == [[16384, 0], [-16384, 0]] and mixer_table(0, 2).tolist() == [[16384, 0]] * 2
    assert mixer_table(1, 4).tolist() == [[16384, 0], [0, 16384], [-16384, 0], [0, -16384]]
    assert mixer_table(3, 4).tolist() == [[16384, 0], [0, -16384], [-16384, 0], [0, 16384]]
    assert mixer_table(2, 4).tolist() == [[16384, 0], [-16384, 0]] * 2
    for k in range(4):
        assert np.array_equal(mixer_table(k, 4), ms.rotation(k))
    assert np.array_equal(mixer_table(7, 4), mixer_table(3, 4))   # k is taken mod N
    for N in (3, 5, 7, 8, 25, 100, 125, 255, 256):
        for k in sorted({0, 1, 2, N // 2, N - 1}):
            w = mixer_table(k, N).astype(np.int64)
            assert w.shape == (N, 2) and np.abs(w).max() <= 16384 and w[0].tolist() == [16384, 0]
            assert np.abs(w - ms.table(k, N)).max() <= 1, (k, N)
            assert np.abs(np.hypot(w[:, 0], w[:, 1]) - 16384).max() <= 1.0
    # capacity and arguments
    buf = (C.c_int16 * 512)()
    assert hip_lib.adsb_mix_table(1, 8, buf, 7) == _lib.ADSB_ERR_CAPACITY and not any(buf)
    assert hip_lib.adsb_mix_table(1, 8, buf, 8) == _lib.ADSB_OK and buf[0] == 16384 and buf[4] == 0 and buf[5] == 16384
    assert hip_lib.adsb_mix_table(1, 0, buf, 256) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_mix_table(1, 257, buf, 256) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_mix_table(1, 8, None, 8) == _lib.ADSB_ERR_INVALID
    with pytest.raises(AdsbError):
        mixer_table(1, 257)


def test_mix_for_shift_on_the_headers_radios(hip_lib):
    from dump1090_rs_amd import _lib, mixer_for_shift
    from dump1090_rs_amd._lib import AdsbError
    for (up, down, hz), want in {
            (1, 4, -2_400_000): (3, 4), (1, 4, 2_400_000): (1, 4), (1, 4, 1_200_000): (1, 8), (1, 2, -1_200_000): (3, 4),
            (6, 25, 2_400_000): (6, 25), (6, 25, -2_400_000): (19, 25), (24, 125, -2_400_000): (101, 125),
            (1, 5, 2_880_000): (6, 25), (1, 10, 2_880_000): (3, 25), (1, 10, -2_400_000): (9, 10), (3, 25, 5_000_000): (1, 4),
            (1, 8, 0): (0, 1), (24, 25, 0): (0, 1), (1, 2, 4_800_000): (0, 1), (1, 16, -150_000): (255, 256)}.items():
        assert mixer_for_shift(up, down, hz) == want, (up, down, hz)
        k, N = want
        assert (hz * up * N - k * 2_400_000 * down) % (2_400_000 * down * N) == 0   # k / N = the shift, mod 1
    # N > 256: refused, the terms still written
    k, N = C.c_uint32(), C.c_uint32()
    assert hip_lib.adsb_mix_for_shift(1, 4, 1_000_000, C.byref(k), C.byref(N)) == _lib.ADSB_OK and (k.value, N.value) == (5, 48)
    assert hip_lib.adsb_mix_for_shift(1, 4, -1, C.byref(k), C.byref(N)) == _lib.ADSB_ERR_INVALID
    assert (k.value, N.value) == (9_599_999, 9_600_000)
    assert hip_lib.adsb_mix_for_shift(1, 16, 100_000, C.byref(k), C.byref(N)) == _lib.ADSB_ERR_INVALID and (k.value, N.value) == (1, 384)
    with pytest.raises(AdsbError) as e:
        mixer_for_shift(24, 125, 1_000)
    assert e.value.status == _lib.ADSB_ERR_INVALID and e.value.terms == (1, 12500)
    for up, down in [(0, 1), (1, 0), (129, 1), (1, 129)]:
        assert hip_lib.adsb_mix_for_shift(up, down, 0, C.byref(k), C.byref(N)) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_mix_for_shift(1, 4, 0, None, C.byref(N)) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_mix_for_shift(1, 4, 0, C.byref(k), None) == _lib.ADSB_ERR_INVALID


def test_argument_errors_that_need_no_device(hip_lib):
    from dump1090_rs_amd import _lib
    table = (C.c_int16 * 8)(16384, 0, 0, 16384, -16384, 0, 0, -16384)
    assert hip_lib.adsb_mix_set_decim(None, table, 4) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_mix_set_resamp(None, table, 4) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_mix_set_decim(None, None, 0) == _lib.ADSB_ERR_INVALID
    assert hip_lib.adsb_mix_get_decim(None) == 0 and hip_lib.adsb_mix_get_resamp(None) == 0


def test_adsb_feed_shift_is_a_usage_error_without_a_filter(hip_lib):
    feed = str(ROOT / "dump1090_rs_amd" / "adsb_feed")
    for args in (["--shift", "-2400000", "x.iq"], ["--shift", "abc", "--decimate", "4", "x.iq"], ["--shift", "--decimate", "4", "x.iq"],
                 ["--decimate", "4", "--shift", "1", "x.iq"], ["--resample", "6/25", "--decimate", "4", "--shift", "0", "x.iq"]):
        r = subprocess.run([feed, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage" in r.stderr and "[--shift HZ]" in r.stderr, args
    r = subprocess.run([feed, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--decimate D | --resample L/M] [--shift HZ]" in r.stderr


# ----------------------------------------------------------------------------------------------- the yardstick itself
def test_restatement_rounds_and_clamps_as_the_definition_says():
    one = np.array([[8192, 0]], np.int16)
    assert ms.mix([[1, 0]], one).tolist() == [[1, 0]]     # (8192 + 8192) >> 14: a half rounds up
    assert ms.mix([[-1, 0]], one).tolist() == [[0, 0]]    # (-8192 + 8192) >> 14
    assert ms.mix([[0, 1]], one).tolist() == [[0, 1]] and ms.mix([[0, -1]], one).tolist() == [[0, 0]]
    assert ms.mix([[32767, 32767]], [[23170, 23170]]).tolist() == [[0, 32767]]   # im = 2 x 32767 x 23170 >> 14 clamps
    assert ms.mix([[32767, -32767]], [[23170, 23170]]).tolist() == [[32767, 0]]
    for c, s in [(32767, 32767), (32767, -32767), (-32767, 32767), (-32767, -32767)]:
        re, im = -32768 * c - 32767 * s, -32768 * s + 32767 * c
        want = [min(max((v + 8192) >> 14, -32768), 32767) for v in (re, im)]
        assert abs(re) < 2 ** 31 - 8192 and abs(im) < 2 ** 31 - 8192
        assert ms.mix([[-32768, 32767]], [[c, s]]).tolist() == [want]
    assert ms.mix([[5, -7]], [[16384, 0]]).tolist() == [[5, -7]]
    assert ms.mix([[5, -7]] * 3, None).tolist() == [[5, -7]] * 3


def test_restatement_rotate_and_counter_rotate_is_the_identity_at_n_4():
    rng = np.random.default_rng(4)
    x = rng.integers(-32767, 32768, size=(1001, 2), dtype=np.int64).astype(np.int16)
    for P in (0, 1, 2, 3, 1001):
        there = ms.mix(x, ms.rotation(1), P)
        assert not np.array_equal(there, x)
        assert np.array_equal(ms.mix(there, ms.rotation(3), P), x)
        assert np.array_equal(np.abs(there.astype(np.int64)).sum(axis=1), np.abs(x.astype(np.int64)).sum(axis=1))
    # and a sample of -32768 is where it stops being one: j x (-32768 + 0 j) has no int16
    assert ms.mix(ms.mix([[0, -32768]], ms.rotation(1), 1), ms.rotation(3), 1).tolist() == [[0, -32767]]


def test_restatement_applies_the_table_by_absolute_index():
    rng = np.random.default_rng(5)
    x = rs.random_iq(rng, 700, run=9)
    for N in (1, 3, 7, 256):
        w = ms.random_table(rng, N)
        assert np.abs(w.astype(np.int64)).max() == 32767
        whole = ms.mix(x, w, 0)
        parts, at = [], 0
        for n in [0, 1, 2, N - 1, N, N + 1, 300, 700]:
            n = min(n, len(x) - at)
            parts.append(ms.mix(x[at:at + n], w, at))
            at += n
        assert np.array_equal(np.concatenate(parts), whole)


@pytest.mark.parametrize("D, T, s, N", [(2, 17, 15, 4), (5, 41, 15, 25), (16, 512, 16, 7)])
def test_restatement_streams_are_cut_invariant_and_compositional(D, T, s, N):
    rng = np.random.default_rng(100 * D + N)
    h = ds.random_taps(rng, T)
    hr = rs.random_phase_taps(rng, T, 3)
    w = ms.random_table(rng, N)
    x = rs.random_iq(rng, 2600, run=T)
    want_d, want_r = ms.decimate(x, h, D, s, w), ms.resample(x, hr, 3, D, s, w)
    assert np.array_equal(want_d, ds.decimate(ms.mix(x, w), h, D, s))
    a, b = ms.DecimStream(h, D, s, w), ms.ResampStream(hr, 3, D, s, w)
    got_d, got_r, at = [], [], 0
    for n in rs.cut_plan(rng, len(x), [0, 1, 2, N - 1, N + 1, T - 2, T, 999], D):
        got_d.append(a.run(x[at:at + n]))
        got_r.append(b.run(x[at:at + n]))
        at += n
    assert np.array_equal(np.concatenate(got_d), want_d) and np.array_equal(np.concatenate(got_r), want_r)
    # a schedule: on, changed, off -- the history holds mixed samples, the table goes by the absolute index
    w2 = ms.random_table(rng, N + 1)
    a.reset()
    cuts, tabs = [0, 100, 100 + T // 2, 900, 2600], [w, w2, None, w]
    parts, mixed = [], []
    for (lo, hi), tab in zip(zip(cuts, cuts[1:]), tabs):
        a.set_mixer(tab)
        parts.append(a.run(x[lo:hi]))
        mixed.append(ms.mix(x[lo:hi], tab, lo))
    assert np.array_equal(np.concatenate(parts), ds.decimate(np.concatenate(mixed), h, D, s))
