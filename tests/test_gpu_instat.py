"""Input statistics on the device (include/adsb_hip.h, "Input statistics"): the record a decimator, a resampler or a bank
counts on its raw input, held field for field to the numpy restatement of the definition (tests/instat_support.py, with
tests/formats_in_support.py for the conversion) -- never to anything taken from the library.  Where outputs are compared,
they are held to the existing restatements (tests/resamp_support.py, tests/decim_support.py, tests/mix_support.py):
the filter's outputs are what they are with the mode off.  Tolerance 0 everywhere.

t = tile_samples and G = max_groups_per_run of adsb_instat_selftest_geometry: a run longer than G t gives a workgroup a
second tile.  Every device input is followed by 64 samples of rail values (CF32: NaN) that no record may count."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import decim_support as ds
from tests import formats_in_support as fi
from tests import instat_support as ist
from tests import mix_support as ms
from tests import resamp_support as rs
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CHUNK = 131072
CS16, U8, CF32, REAL16 = ist.CS16, ist.U8, ist.CF32, ist.REAL16
CANARY = 0x5A5A
PAD = 64


def t_soapy() -> np.ndarray:
    x = np.arange(256, dtype=np.float32)
    return np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)


def geometry(hip_lib, fmt: int):
    t, g = C.c_uint32(), C.c_uint32()
    assert hip_lib.adsb_instat_selftest_geometry(fmt, C.byref(t), C.byref(g)) == 0
    assert t.value >= 64 and g.value >= 2
    return int(t.value), int(g.value)


@pytest.fixture()
def ctx(hip_lib):
    """A context whose input is ordered behind a torch stream (adsb_set_stream), with T_soapy set as its 8-bit table."""
    import torch
    from dump1090_rs_amd import Context
    with Context(0, 1) as c:
        c.torch_stream = torch.cuda.Stream()
        c.set_stream(c.torch_stream.cuda_stream)
        c.set_u8_table(t_soapy())
        yield c
        torch.cuda.synchronize()


def upload(x, fmt: int):
    """x followed by PAD samples that must never be counted, on the device."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([x, ist.rail_fill(fmt, PAD)]))).cuda()


def run(handle, x, fmt: int = CS16, cap=None) -> np.ndarray:
    """One *_run_device call on x -> its outputs, (n_out, 2) int16."""
    import torch
    want_n = handle.out_count(len(x))
    cap = want_n if cap is None else cap
    with torch.cuda.stream(handle._ctx.torch_stream):
        d_in = upload(x, fmt)
        d_out = torch.full((max(cap, 1) + 8, 2), CANARY, dtype=torch.int16, device="cuda")
        n = handle.run_device(d_in.data_ptr(), len(x), d_out.data_ptr(), cap, format=fmt)
        assert n == want_n
        y = d_out.cpu().numpy()
    assert (y[n:] == CANARY).all()
    return y[:n]


def assert_record(got, want, what=None):
    assert ist.same(got, want), (what, ist.explain(np.asarray(got, ist.DTYPE), want))


def launches(hip_lib, handle, kind: str) -> int:
    return int(getattr(hip_lib, f"adsb_instat_selftest_launches_{kind}")(handle._h))


def make(ctx, which: str):
    """(handle, kind) of the three handles test 1 names."""
    if which == "plain":
        return ctx.resampler(1, 1, [1], 0), "resamp"
    if which == "3/25":
        return ctx.resampler(3, 25), "resamp"
    return ctx.decimator(2), "decim"


# ----------------------------------------------------------------------------------------------- 1. every size
@pytest.mark.parametrize("which", ["plain", "3/25", "D=2"])
@pytest.mark.parametrize("fmt", [CS16, U8, CF32, REAL16])
def test_every_size(hip_lib, ctx, fmt, which):
    t, G = geometry(hip_lib, fmt)
    rng = np.random.default_rng(11000 + 10 * fmt + len(which))
    handle, kind = make(ctx, which)
    with handle:
        handle.set_input_stats(True)
        assert handle.input_stats_enabled
        for i, n in enumerate([1, 2, 3, 7, t - 1, t, t + 1, 2 * t + 3, G * t + 5]):
            x = ist.sprinkled(rng, fmt, n)
            run(handle, x, fmt)
            want = ist.record(x, fmt, table=t_soapy())
            assert want["n_samples"] == n
            assert_record(handle.input_stats(), want, (fmt, which, n))
            assert launches(hip_lib, handle, kind) == i + 1
        assert_record(handle.input_stats(), ist.empty(), "a second fetch")


# ----------------------------------------------------------------------------------------------- 2. edge values
def test_edge_values(hip_lib, ctx):
    import torch
    v = np.array([-32768, -32767, -1, 0, 1, 32766, 32767], np.int16)
    cs16 = np.ascontiguousarray(np.stack(np.meshgrid(v, v, indexing="ij"), axis=-1).reshape(-1, 2))
    b = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    u8 = np.concatenate([np.stack(np.meshgrid(b, b, indexing="ij"), axis=-1).reshape(-1, 2), np.array([[7, 7], [7, 1], [1, 7]], np.uint8)])
    table = (np.arange(256, dtype=np.int64) * 97 % 30011 - 15000).astype(np.int16)
    table[0], table[255], table[7] = 5, -7, 32767     # the bytes decide clipping, not the table
    e = fi.edge_values()
    cf32 = np.concatenate([np.stack([e, e[::-1]], axis=1), np.stack([e, np.roll(e, 5)], axis=1),
                           np.array([[np.nan, np.inf], [-np.inf, np.nan], [np.nan, np.nan], [np.nan, 0.25]], np.float32)]).astype(np.float32)
    real = np.array([-32768, 32767, 0, 1, -1, 32766, -32767, 5, 32767], np.int16)   # odd; the int16 behind it is a rail
    assert len(real) % 2 == 1 and ist.rail_fill(REAL16, 1)[0] in ist.RAILS
    with ctx.resampler(1, 1, [1], 0) as res:
        res.set_input_stats(True)
        run(res, cs16, CS16)
        want = ist.record(cs16, CS16)
        assert want["n_clipped"] == 49 - 25 and want["peak"] == 32768 and want["hist"][16] == 14 and want["hist"][0] == 14
        assert_record(res.input_stats(), want, "CS16")
        torch.cuda.synchronize()
        ctx.set_u8_table(table)
        try:
            run(res, u8, U8)
            want = ist.record(u8, U8, table=table)
            assert want["n_clipped"] == 36 - 16 and want["peak"] == 32767 and want["hist"][15] >= 3
            assert_record(res.input_stats(), want, "8-bit")
        finally:
            torch.cuda.synchronize()
            ctx.set_u8_table(t_soapy())
        for g in (32768.0, fi.G2):
            res.set_scale(g)
            run(res, cf32, CF32)
            want = ist.record(cf32, CF32, g=g)
            # n_nan and n_clipped held apart: a NaN is never a rail, an infinity beside a NaN still is
            n_nan = int(np.isnan(cf32).any(axis=1).sum())
            assert want["n_nan"] == n_nan and n_nan >= 6 and want["n_clipped"] > 0
            only_nan = ist.record(cf32[-2:], CF32, g=g)
            assert only_nan["n_nan"] == 2 and only_nan["n_clipped"] == 0 and only_nan["hist"][0] == 3
            assert ist.record(cf32[-4:-2], CF32, g=g)["n_clipped"] == 2
            assert_record(res.input_stats(), want, ("CF32", g))
        run(res, real, REAL16)
        want = ist.record(real, REAL16)
        assert want["n_samples"] == 9 and want["n_clipped"] == 3 and want["hist"].sum() == 9 and want["sum_im2"] == 0
        assert_record(res.input_stats(), want, "REAL16")


# ----------------------------------------------------------------------------------------------- 3. worst-case magnitudes
def test_worst_case_magnitudes(hip_lib, ctx):
    t, _ = geometry(hip_lib, CS16)
    n = 2 * t + 3
    with ctx.resampler(1, 1, [1], 0) as res:
        res.set_input_stats(True)
        for re, im in [(-32768, -32768), (32767, -32768)]:
            x = np.tile(np.array([[re, im]], np.int16), (n, 1))
            run(res, x, CS16)
            got = res.input_stats()
            assert got["n_samples"] == n and got["n_clipped"] == n and got["peak"] == 32768
            assert got["sum_re"] == n * re and got["sum_im"] == n * im                 # signs
            assert got["sum_re2"] == n * re * re and got["sum_im2"] == n * im * im     # a 32-bit partial wraps at four samples
            assert got["sum_re_im"] == n * re * im
            assert got["hist"][16] == (2 * n if re == -32768 else n) and got["hist"][15] == (0 if re == -32768 else n)
            assert_record(got, ist.record(x, CS16), (re, im))


# ----------------------------------------------------------------------------------------------- 4. the cut is invisible
def play_stream(hip_lib, ctx, handle, kind, ref, K: int, mixers, rng):
    """The ragged calls of test 4 on one handle -> (records fetched, records expected).  `mixers`: call index -> table
    (None clears) set in front of that call, on the handle and on the restatement alike."""
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd._lib import AdsbError
    fmts = [CS16, CF32, U8, REAL16]
    t = {f: geometry(hip_lib, f)[0] for f in fmts}
    lens = lambda f: [0, 1, K - 2, t[f] + 1, 2 * t[f] + 3, t[f] + 1, 2 * t[f] + 3, 1]   # noqa: E731
    handle.set_scale(fi.G2)
    handle.set_input_stats(True)
    got, want, acc = [], [], ist.empty()
    n_launches = 0
    for i in range(8):
        f = fmts[i % 4]
        n = lens(f)[i]
        if i in mixers:
            handle.set_mixer(mixers[i])
            ref.set_mixer(mixers[i])
        x = ist.sprinkled(rng, f, n, fi.G2)
        if i == 3:
            # refused: nothing consumed, nothing counted, nothing launched
            with pytest.raises(AdsbError) as e:
                run(handle, x, f, cap=handle.out_count(n) - 1)
            assert e.value.status == _lib.ADSB_ERR_CAPACITY
            assert launches(hip_lib, handle, kind) == n_launches
        y = run(handle, x, f)
        n_launches += n > 0
        assert launches(hip_lib, handle, kind) == n_launches   # a run of no input counts nothing
        assert np.array_equal(y, ref.run(fi.to_cs16(x, f, fi.G2, t_soapy()))), (kind, i)
        acc = ist.add(acc, ist.record(x, f, g=fi.G2, table=t_soapy()))
        if i == 2 or i == 7:
            got.append(handle.input_stats())
            want.append(acc)
            acc = ist.empty()
    return got, want


@pytest.mark.parametrize("kind", ["resamp", "decim"])
def test_the_cut_is_invisible_formats_alternating(hip_lib, ctx, kind):
    from dump1090_rs_amd import default_resampler_taps, default_taps
    w1, w2 = ms.random_table(np.random.default_rng(1), 7), ms.random_table(np.random.default_rng(2), 5)
    records = []
    for mixers in ({1: w1, 4: w2, 6: None}, {}):
        rng = np.random.default_rng(12000)   # the same inputs with the mixer and without
        if kind == "resamp":
            h, s = default_resampler_taps(6, 5)
            handle, ref, K = ctx.resampler(6, 5, h, s), ms.ResampStream(h, 6, 5, s), rs.phase_taps(6, len(h))
        else:
            h, s = default_taps(5)
            handle, ref, K = ctx.decimator(5, h, s), ms.DecimStream(h, 5, s), len(h)
        with handle:
            got, want = play_stream(hip_lib, ctx, handle, kind, ref, K, mixers, rng)
        assert len(got) == 2 and want[0]["n_samples"] == 1 + K - 2
        for g, w in zip(got, want):
            assert_record(g, w, (kind, bool(mixers)))
        records.append(got)
    assert all(ist.same(a, b) for a, b in zip(*records))   # the mixer does not enter


# ----------------------------------------------------------------------------------------------- 5. off means off
@pytest.mark.parametrize("kind", ["resamp", "decim"])
def test_off_means_off(hip_lib, ctx, kind):
    from dump1090_rs_amd import _lib, default_resampler_taps, default_taps
    from dump1090_rs_amd._lib import AdsbError
    rng = np.random.default_rng(13000)
    if kind == "resamp":
        h, s = default_resampler_taps(3, 25)
        handle, ref = ctx.resampler(3, 25, h, s), rs.Stream(h, 3, 25, s)
    else:
        h, s = default_taps(2)
        handle, ref = ctx.decimator(2, h, s), ds.Stream(h, 2, s)
    xs = [ist.sprinkled(rng, CS16, n) for n in (700, 5000, 333, 4097, 900, 1200)]
    with handle:
        assert not handle.input_stats_enabled
        assert np.array_equal(run(handle, xs[0]), ref.run(xs[0]))
        assert launches(hip_lib, handle, kind) == 0
        with pytest.raises(AdsbError) as e:
            handle.input_stats()
        assert e.value.status == _lib.ADSB_ERR_INVALID
        handle.set_input_stats(True)
        handle.set_input_stats(True)   # (already on: changes nothing)
        assert np.array_equal(run(handle, xs[1]), ref.run(xs[1]))
        assert launches(hip_lib, handle, kind) == 1
        handle.set_input_stats(False)
        assert not handle.input_stats_enabled
        assert np.array_equal(run(handle, xs[2]), ref.run(xs[2]))
        assert launches(hip_lib, handle, kind) == 1
        with pytest.raises(AdsbError):
            handle.input_stats()
        handle.set_input_stats(True)
        assert np.array_equal(run(handle, xs[3]), ref.run(xs[3]))
        handle.reset()   # the stream starts over; the record does not
        ref.reset()
        assert np.array_equal(run(handle, xs[4]), ref.run(xs[4]))
        assert launches(hip_lib, handle, kind) == 3
        # only what came after the last enable
        assert_record(handle.input_stats(), ist.add(ist.record(xs[3], CS16), ist.record(xs[4], CS16)), kind)
        assert np.array_equal(run(handle, xs[5]), ref.run(xs[5]))
        assert_record(handle.input_stats(), ist.record(xs[5], CS16), kind)


# ----------------------------------------------------------------------------------------------- 6. bank
def bank_call(ctx, bank, call, fmt: int):
    """One adsb_bank_run_device call over [(stream, input)] -> the outputs, each (n_out, 2) int16."""
    import torch
    with torch.cuda.stream(ctx.torch_stream):
        d_in = [upload(x, fmt) for _, x in call]
        n_want = [bank.out_count(s, len(x)) for s, x in call]
        d_out = [torch.full((n + 8, 2), CANARY, dtype=torch.int16, device="cuda") for n in n_want]
        n = bank.run_device([s for s, _ in call], [d.data_ptr() for d in d_in], [len(x) for _, x in call],
                            [d.data_ptr() for d in d_out], n_want, format=fmt)
        assert n.tolist() == n_want
        ys = [d.cpu().numpy() for d in d_out]
    for y, k in zip(ys, n_want):
        assert (y[k:] == CANARY).all()
    return [y[:k] for y, k in zip(ys, n_want)]


@pytest.mark.parametrize("L, M", [(3, 25), (33, 17)])
def test_bank_ragged_calls(hip_lib, ctx, L, M):
    from dump1090_rs_amd import _lib, default_resampler_taps
    from dump1090_rs_amd._lib import AdsbError
    h, s = default_resampler_taps(L, M)
    N = 5
    fmts = [CS16, CF32, REAL16, U8]
    rng = np.random.default_rng(14000 + L)
    refs = [rs.Stream(h, L, M, s) for _ in range(N)]
    acc = [ist.empty() for _ in range(N)]
    with ctx.resampler_bank(N, L, M, h, s) as bank:
        with pytest.raises(AdsbError) as e:
            bank.input_stats()
        assert e.value.status == _lib.ADSB_ERR_INVALID
        bank.set_input_stats(True)
        for i, fmt in enumerate(fmts):
            t = geometry(hip_lib, fmt)[0]
            lens = [[1, t - 1, t + 1, 7, 2 * t + 3][(k + i) % 5] for k in range(N)]
            streams = [int(k) for k in rng.permutation(N)]
            if i == 1:
                streams.remove(3)     # a stream left out of a call
            if i == 2:
                lens[0] = 0           # a run of no input
            call = [(k, ist.sprinkled(rng, fmt, lens[k])) for k in streams]
            ys = bank_call(ctx, bank, call, fmt)
            for (k, x), y in zip(call, ys):
                assert np.array_equal(y, refs[k].run(fi.to_cs16(x, fmt, table=t_soapy()))), (i, k)
                acc[k] = ist.add(acc[k], ist.record(x, fmt, table=t_soapy()))
            assert launches(hip_lib, bank, "bank") == i + 1
            if i == 1:
                # streams 1 .. 2 fetched: only those start over
                got = bank.input_stats(1, 2)
                assert got.shape == (2,)
                for k in (1, 2):
                    assert_record(got[k - 1], acc[k], (i, k))
                    acc[k] = ist.empty()
        got = bank.input_stats()
        assert got.shape == (N,)
        for k in range(N):
            assert_record(got[k], acc[k], k)
        assert all(ist.same(r, ist.empty()) for r in bank.input_stats())
        for first, n in [(N, 1), (0, N + 1), (N + 1, 0)]:
            with pytest.raises(AdsbError):
                bank.input_stats(first, n)


def test_bank_of_300_tiny_runs(hip_lib, ctx):
    import torch
    from dump1090_rs_amd import default_resampler_taps
    L, M, N, SLOT = 3, 25, 300, 4   # a 16-byte slot per stream
    h, s = default_resampler_taps(L, M)
    rng = np.random.default_rng(14500)
    n_in = 1 + np.arange(N) % 3
    x = ist.sprinkled(rng, CS16, N * SLOT).reshape(N, SLOT, 2)
    for k in range(N):
        x[k, n_in[k]:] = -32768   # behind every run: rails that are never counted
    with ctx.resampler_bank(N, L, M, h, s) as bank:
        bank.set_input_stats(True)
        with torch.cuda.stream(ctx.torch_stream):
            d_in = torch.from_numpy(x.reshape(-1, 2)).cuda()
            d_out = torch.full((N * SLOT, 2), CANARY, dtype=torch.int16, device="cuda")
            order = np.arange(N)[::-1].copy()
            bank.run_device(order, d_in.data_ptr() + order * (SLOT * 4), n_in[order], d_out.data_ptr() + order * (SLOT * 4),
                            np.full(N, SLOT))
        got = bank.input_stats()
        for k in range(N):
            assert_record(got[k], ist.record(x[k, : n_in[k]], CS16), k)
        assert launches(hip_lib, bank, "bank") == 1


def test_bank_uneven_grid(hip_lib, ctx):
    from dump1090_rs_amd import default_resampler_taps
    L, M = 3, 25
    h, s = default_resampler_taps(L, M)
    t, G = geometry(hip_lib, CS16)
    rng = np.random.default_rng(14600)
    lens = [t - 1, t - 1, G * t + 5, t - 1, t - 1]
    call = [(k, ist.sprinkled(rng, CS16, n)) for k, n in enumerate(lens)]
    with ctx.resampler_bank(5, L, M, h, s) as bank:
        bank.set_input_stats(True)
        ys = bank_call(ctx, bank, call, CS16)
        got = bank.input_stats()
        for (k, x), y in zip(call, ys):
            assert_record(got[k], ist.record(x, CS16), k)
            if len(x) < t:
                assert np.array_equal(y, rs.resample(x, h, L, M, s)), k


# ----------------------------------------------------------------------------------------------- 7. the blocking host form
def test_the_blocking_host_form(hip_lib, golden, fixture_iq):
    from dump1090_rs_amd import Context
    fx = next(f for f in golden["fixtures"] if f["file"] == "test_1641427457780.iq")
    iq = fixture_iq[fx["file"]]
    with Context(0, 1) as c:
        x = np.repeat(iq, 2, axis=0)
        with c.decimator(2, [1], 0) as dec:
            dec.set_input_stats(True)
            c.icao_flush()
            got = dec.demod_iq(x)
            assert [m.buffer().hex() for m in got] == fx["frames"] and len(got) in (5, 6)
            assert [m.j for m in got] == fx["j"] and [m.try_phase for m in got] == fx["try_phase"]
            rec = dec.input_stats()
            assert rec["n_samples"] == len(x)
            assert_record(rec, ist.record(x, CS16), "decimator")
        f = fi.cs16_as_cf32(iq)
        with c.resampler(1, 1, [1], 0) as res:
            res.set_input_stats(True)
            c.icao_flush()
            got = res.demod_iq(f, format=CF32)
            assert [m.buffer().hex() for m in got] == fx["frames"]
            rec = res.input_stats()
            assert rec["n_samples"] == len(f)
            assert_record(rec, ist.record(f, CF32), "resampler, CF32")
            assert_record(rec, ist.record(iq, CS16), "q brings the capture back")


# ----------------------------------------------------------------------------------------------- 8. adsb_feed
def test_adsb_feed_input_stats(hip_lib, golden, fixture_iq, tmp_path):
    from dump1090_rs_amd import input_summary
    fx = next(f for f in golden["fixtures"] if f["file"] == "test_1641427457780.iq")
    x = np.repeat(fixture_iq[fx["file"]], 2, axis=0)
    path = tmp_path / "x2.iq"
    np.ascontiguousarray(x[:, ::-1]).astype("<i2").tofile(path)   # the capture format: im first
    feed = str(ROOT / "dump1090_rs_amd" / "adsb_feed")
    plain = subprocess.run([feed, "--decimate", "2", "--buffers", "2", str(path)], capture_output=True, timeout=120)
    with_stats = subprocess.run([feed, "--decimate", "2", "--buffers", "2", "--input-stats", str(path)], capture_output=True, timeout=120)
    assert plain.returncode == 0 and with_stats.returncode == 0, with_stats.stderr
    assert with_stats.stdout == plain.stdout and len(plain.stdout) > 0
    assert b"input stats" not in plain.stderr
    lines = [ln for ln in with_stats.stderr.decode().splitlines() if ln.startswith("adsb_feed: input stats (whole input)")]
    assert lines
    s = input_summary(ist.record(x, CS16))
    assert s["n_samples"] == len(x)
    want = ("adsb_feed: input stats (whole input): samples %d, mean %.3f dBFS, peak %.3f dBFS, dc re %.3f im %.3f LSB, "
            "clipped %.6f %%, nan %.6f %%, iq gain %.3f dB, bits %d" % (
                s["n_samples"], s["mean_power_dbfs"], s["peak_dbfs"], s["dc_re"], s["dc_im"], 100.0 * s["clipped_fraction"],
                100.0 * s["nan_fraction"], s["iq_gain_db"], s["bits_used"]))
    assert lines[-1] == want
    # only in front of a filter
    alone = subprocess.run([feed, "--input-stats", str(path)], capture_output=True, timeout=120)
    assert alone.returncode == 2 and alone.stdout == b""
