"""CF32 and REAL16 input of the decimator and the resampler on the device (include/adsb_hip.h, "Sample formats"), held bit
for bit to the numpy restatement of the conversion (tests/formats_in_support.py) followed by the restated mixer and
filters, and its frames to the reference's and the CPU oracle's.  Shapes are a few tiles of t = adsb_*_selftest_tile
outputs plus a ragged end.  Every comparison is at tolerance 0."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import decim_support as ds
from tests import formats_in_support as fi
from tests import mix_support as ms
from tests import resamp_support as rs
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CHUNK = 131072
CS16, U8, CF32, REAL16 = fi.CS16, fi.U8, fi.CF32, fi.REAL16
NEW = [CF32, REAL16]
NAME = {CS16: "cs16", U8: "8bit", CF32: "cf32", REAL16: "real16"}


def t_soapy() -> np.ndarray:
    x = np.arange(256, dtype=np.float32)
    return np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)


def key(m):
    return (m.chunk, m.j, m.try_phase, m.score, m.msglen, m.msg.hex(), m.signal_level)


def assert_same(msgs, want):
    exp = [(w["chunk"], w["j"], w["try_phase"], w["score"], w["len"], w["msg"].hex(), w["signal_level"]) for w in want]
    assert [key(m) for m in msgs] == exp


@pytest.fixture()
def ctx(hip_lib):
    """A context whose input is ordered behind a torch stream (adsb_set_stream): run() copies in, filters and reads back
    in that stream's order, with no other synchronisation."""
    import torch
    from dump1090_rs_amd import Context
    with Context(0, 1) as c:
        c.torch_stream = torch.cuda.Stream()
        c.set_stream(c.torch_stream.cuda_stream)
        yield c
        torch.cuda.synchronize()


def run(h, x: np.ndarray, fmt: int, n_in=None) -> np.ndarray:
    """One *_run_device call of a decimator or resampler on the first n_in samples of x (all of them by default; what
    lies behind them is in the allocation, not in the call) -> its outputs, (n_out, 2) int16."""
    import torch
    n_in = len(x) if n_in is None else n_in
    want_n = h.out_count(n_in)
    with torch.cuda.stream(h._ctx.torch_stream):
        d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        d_out = torch.full((max(want_n, 1) + 8, 2), 0x5A5A, dtype=torch.int16, device="cuda")
        n = h.run_device(d_in.data_ptr(), n_in, d_out.data_ptr(), want_n, format=fmt)
        assert n == want_n
        y = d_out.cpu().numpy()
    assert (y[n:] == 0x5A5A).all()   # the canary: nothing written behind the call's outputs
    return y[:n]


def random_input(rng, n: int, fmt: int, table=None) -> np.ndarray:
    """n samples in `fmt`, full range.  CF32: values of up to 1.1 full scale between the int16 steps, so that the
    rounding and both rails take part, with every edge value of q among them."""
    if fmt == CS16:
        return rs.random_iq(rng, n)
    if fmt == U8:
        return rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
    if fmt == REAL16:
        r = rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16)
        r[rng.integers(0, n, size=max(n // 50, 1))] = rng.choice([-32768, 32767], size=max(n // 50, 1))
        return r
    f = rng.uniform(-1.1, 1.1, size=(n, 2)).astype(np.float32)
    half = (rng.integers(-32768, 32768, size=(n, 2)) + 0.5) / 32768   # ties at the default scale
    f = np.where(rng.random((n, 2)) < 0.1, half.astype(np.float32), f)
    edges = fi.edge_values()
    at = rng.integers(0, n, size=len(edges))
    f[at, rng.integers(0, 2, size=len(edges))] = edges
    return np.ascontiguousarray(f)


# (name, L, M, decimator?, taps, shift): the issue's configurations
def configs(rng):
    return [("D2/17", 1, 2, True, ds.random_taps(rng, 17), 16),
            ("D5/default", 1, 5, True, ds.hamming_sinc_taps(5), 15),
            ("D16/512", 1, 16, True, ds.random_taps(rng, 512), 16),   # the CF32 register and LDS extreme
            ("6/5", 6, 5, False, rs.hamming_sinc_taps(6, 5), 14),
            ("24/25", 24, 25, False, rs.hamming_sinc_taps(24, 25), 14),
            ("3/25", 3, 25, False, rs.hamming_sinc_taps(3, 25), 14),
            ("1/1 one tap", 1, 1, False, np.array([1], np.int16), 0)]


def device(ctx, L, M, decim, h, s):
    return ctx.decimator(M, h, s) if decim else ctx.resampler(L, M, h, s)


def restated(L, M, decim, h, s):
    return ms.DecimStream(h, M, s) if decim else ms.ResampStream(h, L, M, s)


def tile_of(lib, L, M, decim) -> int:
    return int(lib.adsb_decim_selftest_tile()) if decim else int(lib.adsb_resamp_selftest_tile(L, M))


# ----------------------------------------------------------------------------------------------- 0. the calls exist
@pytest.mark.parametrize("fmt", NEW, ids=[NAME[f] for f in NEW])
def test_the_four_calls_take_the_format(hip_lib, fmt):
    """adsb_decim_run_device, adsb_decim_demod_iq, adsb_resamp_run_device and adsb_resamp_demod_iq with a new format:
    ADSB_OK (ADSB_ERR_INVALID before the formats existed), on an empty and on a short input."""
    import torch
    from dump1090_rs_amd import Context, _lib
    x = random_input(np.random.default_rng(fmt), 40, fmt)
    n, out = C.c_size_t(), (_lib.AdsbMsg * 16)()
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros((64, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with Context(0, 1) as c, c.decimator(2, [1, 1], 0) as dec, c.resampler(1, 1, [1], 0) as res:
        for h, run_device, demod in ((dec, hip_lib.adsb_decim_run_device, hip_lib.adsb_decim_demod_iq),
                                     (res, hip_lib.adsb_resamp_run_device, hip_lib.adsb_resamp_demod_iq)):
            assert run_device(h._h, fmt, None, 0, C.c_void_p(d_out.data_ptr()), 64, C.byref(n)) == _lib.ADSB_OK and n.value == 0
            assert run_device(h._h, fmt, C.c_void_p(d_in.data_ptr()), 40, C.c_void_p(d_out.data_ptr()), 64, C.byref(n)) == _lib.ADSB_OK
            assert n.value == (20 if h is dec else 40)
            assert run_device(h._h, 4, C.c_void_p(d_in.data_ptr()), 40, C.c_void_p(d_out.data_ptr()), 64, C.byref(n)) == _lib.ADSB_ERR_INVALID
            assert run_device(h._h, -1, C.c_void_p(d_in.data_ptr()), 40, C.c_void_p(d_out.data_ptr()), 64, C.byref(n)) == _lib.ADSB_ERR_INVALID
            assert demod(h._h, fmt, None, 0, out, 16, C.byref(n)) == _lib.ADSB_OK and n.value == 0
            assert demod(h._h, fmt, C.c_void_p(x.ctypes.data), 40, out, 16, C.byref(n)) == _lib.ADSB_OK and n.value == 0
            assert demod(h._h, 4, C.c_void_p(x.ctypes.data), 40, out, 16, C.byref(n)) == _lib.ADSB_ERR_INVALID


# ----------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("N", [0, 4, 125])
@pytest.mark.parametrize("fmt", NEW, ids=[NAME[f] for f in NEW])
def test_exact_against_numpy(hip_lib, ctx, fmt, N):
    rng = np.random.default_rng([1, fmt, N])
    w = None if N == 0 else ms.rotation(1) if N == 4 else ms.random_table(rng, N)
    g = fi.DEFAULT_SCALE if N == 0 else fi.G2   # (the non-power-of-two scale under the mixers)
    for name, L, M, decim, h, s in configs(rng):
        t = tile_of(hip_lib, L, M, decim)
        x = random_input(rng, rs.inputs_for(L, M, 0, 2 * t + 37) + 3, fmt)
        ref = restated(L, M, decim, h, s)
        ref.set_mixer(w)
        with device(ctx, L, M, decim, h, s) as dev:
            dev.set_mixer(w)
            dev.set_scale(g)
            # a short first call, so that the long one starts at a P that is no multiple of D, N or the load's samples
            for lo, hi in ((0, 3), (3, len(x))):
                got = run(dev, x[lo:hi], fmt)
                assert np.array_equal(got, ref.run(fi.to_cs16(x[lo:hi], fmt, g))), (name, NAME[fmt], N, lo)
            assert len(got) >= 2 * t + 36


# ----------------------------------------------------------------------------------------------- 2. q itself
def test_edge_values_of_q_come_out_of_a_single_tap(hip_lib, ctx):
    """1/1 with the tap 1 and shift 0: y[n] = q(x[n]).  Every spelled-out edge value as re, and as im in reverse order."""
    e = fi.edge_values()
    x = np.ascontiguousarray(np.stack([e, e[::-1]], axis=1))
    with ctx.resampler(1, 1, [1], 0) as res, ctx.converter() as conv:
        assert res.scale == 32768.0 == conv.scale and (conv.up, conv.down, conv.taps.tolist(), conv.shift) == (1, 1, [1], 0)
        for column, g in ((1, fi.DEFAULT_SCALE), (2, fi.G2)):
            want = np.array([v[column] for v in fi.Q_EDGES], np.int16)
            res.reset()
            res.set_scale(g)
            assert res.scale == g
            got = run(res, x, CF32)
            assert got[:, 0].tolist() == want.tolist() and got[:, 1].tolist() == want[::-1].tolist()
            assert np.array_equal(got, fi.q(x, g))
        assert np.array_equal(run(conv, x, CF32), fi.q(x))
    # ... and the same values in front of a decimator: the tap on x[n D]
    with ctx.decimator(2, [1], 0) as dec:
        assert np.array_equal(run(dec, x, CF32), fi.q(x)[::2])


# ----------------------------------------------------------------------------------------------- 3. cuts
@pytest.mark.parametrize("vary", [False, True], ids=["fixed", "scale-and-mixer-change"])
@pytest.mark.parametrize("name, L, M, decim", [("D5", 1, 5, True), ("3/25", 3, 25, False), ("6/5", 6, 5, False)])
def test_the_cut_is_invisible_and_the_formats_alternate(hip_lib, ctx, name, L, M, decim, vary):
    """One stream cut into calls of 0, 1, 7, fewer than T - 1 and several tiles of samples, the four formats taking
    turns: the concatenated output is the one-call CS16 result on the underlying samples.  `vary`: the scale changes
    from call to call and the mixer is set, changed and cleared between calls -- the restatement is applied per call."""
    rng = np.random.default_rng([3, L, M, vary])
    t = tile_of(hip_lib, L, M, decim)
    h, s = (ds.hamming_sinc_taps(M), 15) if decim else (rs.hamming_sinc_taps(L, M), 14)
    H = rs.phase_taps(L, len(h)) - 1
    total = rs.inputs_for(L, M, 0, 3 * t + 11)
    lengths = [0, 1, 7, H - 2, H + 3, (t + 5) * M // L, (2 * t) * M // L + 1]
    plan = [n for n in (0, 1, 7, H - 2) for _ in range(4)] + [int(n) for n in rng.permutation(lengths)]   # each format takes each
    while sum(plan) < total:
        plan.append(int(rng.choice(lengths)))
    table = t_soapy()
    assert np.array_equal(ctx.u8_table(), table)   # (the context's default)
    scales = [fi.DEFAULT_SCALE, fi.G2, 4096.0] if vary else [fi.DEFAULT_SCALE]
    mixers = [None, ms.rotation(1), ms.random_table(rng, 125), None] if vary else [ms.random_table(rng, 125)]
    ref = restated(L, M, decim, h, s)
    seen, got, under = set(), [], []
    with device(ctx, L, M, decim, h, s) as dev, device(ctx, L, M, decim, h, s) as whole:
        for i, n in enumerate(plan):
            fmt, g, w = (CS16, U8, CF32, REAL16)[i % 4], scales[i % len(scales)], mixers[(i // 3) % len(mixers)]
            x = random_input(rng, n, fmt) if n else random_input(rng, 1, fmt)[:0]
            xc = fi.to_cs16(x, fmt, g, table)
            dev.set_scale(g)
            dev.set_mixer(w)
            ref.set_mixer(w)
            mixed_from = ref.P
            y = run(dev, x, fmt)
            assert np.array_equal(y, ref.run(xc)), (i, n, NAME[fmt])
            got.append(y)
            under.append(xc if not vary else ms.mix(xc, w, mixed_from))
            seen.add((fmt, n))
        assert all((f, n) in seen for f in (CS16, U8, CF32, REAL16) for n in (0, 1, 7, H - 2))
        under = np.concatenate(under)
        if vary:   # (the per-call mixers are in `under` already)
            want = ds.decimate(under, h, M, s) if decim else rs.resample(under, h, L, M, s)
        else:
            want = ms.decimate(under, h, M, s, mixers[0]) if decim else ms.resample(under, h, L, M, s, mixers[0])
            whole.set_mixer(mixers[0])
            assert np.array_equal(run(whole, under, CS16), want)   # the one-call CS16 result, from the device too
        assert np.array_equal(np.concatenate(got), want)


# ----------------------------------------------------------------------------------------------- 4. by position
@pytest.mark.parametrize("name, L, M, decim", [("D2", 1, 2, True), ("6/5", 6, 5, False)])
def test_what_lies_behind_the_end_of_the_call_never_reaches_the_filter(hip_lib, ctx, name, L, M, decim):
    rng = np.random.default_rng([4, L, M])
    t = tile_of(hip_lib, L, M, decim)
    h, s = rs.random_phase_taps(rng, 40 * L, L), 16
    H = rs.phase_taps(L, len(h)) - 1
    for fmt in NEW:
        for n_in in (1, 3, H - 4, (t + 9) * M // L | 1):   # odd: the REAL16 load is rounded up to a dword
            x = random_input(rng, n_in + 64, fmt)
            assert n_in % 2 == 1 and n_in != H
            if fmt == REAL16:
                x[n_in:] = 32767
            else:
                x[n_in:] = [np.nan, 1e30]
            nxt = random_input(rng, H + 2 * M, fmt)
            ref = restated(L, M, decim, h, s)
            with device(ctx, L, M, decim, h, s) as dev:
                for w in (None, ms.rotation(1)):
                    dev.reset(), ref.reset()
                    dev.set_mixer(w), ref.set_mixer(w)
                    # the call, then the one behind it: what the history took from the first
                    assert np.array_equal(run(dev, x, fmt, n_in), ref.run(fi.to_cs16(x[:n_in], fmt))), (NAME[fmt], n_in)
                    assert np.array_equal(run(dev, nxt, fmt), ref.run(fi.to_cs16(nxt, fmt))), (NAME[fmt], n_in, "next")


# ----------------------------------------------------------------------------------------------- 5. frames
def test_cf32_captures_through_the_converter_give_the_reference_frames(hip_lib, golden, fixture_iq):
    from dump1090_rs_amd import Context
    rng = np.random.default_rng(5)
    with Context(0, 1) as c, c.converter() as conv, c.resampler(2, 5, [1, 1], 0) as held:
        for fx in golden["fixtures"]:
            cap = fixture_iq[fx["file"]]
            f = fi.cs16_as_cf32(cap)   # / 32768: exact
            c.icao_flush()
            want = c.demod_iq(cap)
            c.icao_flush()
            conv.reset()
            got = conv.demod_iq(f, format=CF32)
            assert [key(m) for m in got] == [key(m) for m in want]
            assert [m.buffer().hex() for m in got] == fx["frames"] and [m.j for m in got] == fx["j"]
            c.icao_flush()
            conv.reset()
            again = conv.demod_iq(f.view(np.complex64).reshape(-1), format=CF32)   # complex64 is the same bytes
            assert [key(m) for m in again] == [key(m) for m in want]
            # the capture held at 2/5 (6 MS/s), as CF32
            x = rs.hold_input(cap, 2, 5, rng)
            assert np.array_equal(rs.resample(x, [1, 1], 2, 5, 0), cap)
            c.icao_flush()
            held.reset()
            got = held.demod_iq(fi.cs16_as_cf32(x), format=CF32)
            assert [m.buffer().hex() for m in got] == fx["frames"] and [m.try_phase for m in got] == fx["try_phase"]


def test_real_sampled_captures_give_the_oracles_frames(hip_lib, oracle_mod, golden, fixture_iq):
    """r[4 n] = re x[n], r[4 n - 1] = im x[n] through the table of 3/4 turn, D = 4, taps [1, 1], shift 0: the capture with
    the im of sample 0 zeroed (tests/test_formats_in_cpu.py shows the oracle's frames on that are the reference's)."""
    from dump1090_rs_amd import Context, mixer_table
    with Context(0, 1) as c, c.decimator(4, [1, 1], 0) as dec:
        dec.set_mixer(mixer_table(3, 4))
        for fx in golden["fixtures"]:
            cap = fixture_iq[fx["file"]]
            y = cap.copy()
            y[0, 1] = 0
            want, _ = oracle_mod.Oracle().demod_iq(y)
            c.icao_flush()
            dec.reset()
            got = dec.demod_iq(fi.real_carrier(cap), format=REAL16)
            assert_same(got, want)
            assert [m.buffer().hex() for m in got] == fx["frames"]


# ----------------------------------------------------------------------------------------------- 6. adsb_feed
def test_adsb_feed_cf32_and_s16real(hip_lib, oracle_mod, golden, fixture_iq, tmp_path):
    from dump1090_rs_amd import default_resampler_taps, default_taps, mixer_table
    feed = str(ROOT / "dump1090_rs_amd" / "adsb_feed")
    cap = fixture_iq[golden["fixtures"][2]["file"]]
    # CF32 at 2.4 MS/s through 1/1 with its default taps
    path = tmp_path / "x.cf32"
    fi.cs16_as_cf32(cap).astype("<f4").tofile(path)
    h, s = default_resampler_taps(1, 1)
    want, _ = oracle_mod.Oracle().demod_iq(rs.resample(cap, h, 1, 1, s))
    assert len(want) > 0
    r = subprocess.run([feed, "--format", "cf32", "--resample", "1/1", "--buffers", "2", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["*" + w["buffer"].hex() + ";" for w in want]
    # ... and scaled: the file holds the int16 values themselves, --scale 1
    cap.astype("<f4").tofile(path)
    r1 = subprocess.run([feed, "--format", "cf32", "--scale", "1", "--resample", "1/1", "--buffers", "2", str(path)], capture_output=True, text=True, timeout=120)
    assert r1.returncode == 0 and r1.stdout == r.stdout
    # real samples at 9.6 MS/s, the band a quarter of the rate above 0
    rpath = tmp_path / "x.s16"
    real = fi.real_carrier(cap)
    real.astype("<i2").tofile(rpath)
    h, s = default_taps(4)
    want, _ = oracle_mod.Oracle().demod_iq(ms.decimate(fi.real_to_cs16(real), h, 4, s, mixer_table(3, 4)))
    assert len(want) > 0
    r = subprocess.run([feed, "--format", "s16real", "--decimate", "4", "--shift", "-2400000", "--buffers", "2", str(rpath)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["*" + w["buffer"].hex() + ";" for w in want]


# ----------------------------------------------------------------------------------------------- 7. the wrappers
def test_python_wrappers_are_strict_and_the_scale_keeps_its_range(hip_lib, ctx):
    from dump1090_rs_amd import Context, _lib
    from dump1090_rs_amd._lib import AdsbError
    with Context(0, 1) as plain, plain.decimator(2, [1, 1], 0) as dec, plain.resampler(6, 5) as res:
        for h, setter in ((dec, hip_lib.adsb_fmt_set_scale_decim), (res, hip_lib.adsb_fmt_set_scale_resamp)):
            assert h.scale == 32768.0
            h.set_scale(1000.1)
            assert h.scale == fi.G2
            for bad in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan"), float(np.nextafter(np.float32(2.0 ** 31), np.float32(np.inf)))):
                with pytest.raises(AdsbError) as e:
                    h.set_scale(bad)
                assert e.value.status == _lib.ADSB_ERR_INVALID and h.scale == fi.G2
                assert setter(h._h, bad) == _lib.ADSB_ERR_INVALID and h.scale == fi.G2
            for good in (2.0 ** 31, float.fromhex("0x1p-149"), 1.0, 32768.0):
                h.set_scale(good)
                assert h.scale == good
            for bad_iq, fmt, exc in ((np.zeros((4, 2), np.float64), CF32, TypeError), (np.zeros((4, 2), np.int16), CF32, TypeError),
                                     (np.zeros(5, np.float32), CF32, ValueError), (np.zeros((4, 3), np.float32), CF32, ValueError),
                                     (np.zeros((2, 2), np.complex64), CF32, ValueError), (np.zeros(4, np.complex128), CF32, TypeError),
                                     (np.zeros((4, 2), np.int16), REAL16, ValueError), (np.zeros(4, np.int32), REAL16, TypeError),
                                     (np.zeros(4, np.float32), REAL16, TypeError), (np.zeros(4, np.int16), 4, ValueError)):
                with pytest.raises(exc):
                    h.demod_iq(bad_iq, format=fmt)
            assert h.demod_iq(np.zeros(64, np.float32), format=CF32) == [] and h.demod_iq(np.zeros(64, np.int16), format=REAL16) == []
    with ctx.converter(scale=4096.0) as conv:
        assert conv.scale == 4096.0
        assert np.array_equal(run(conv, np.array([[0.25, -8.0]], np.float32), CF32), [[1024, -32768]])
