"""The mixer of the decimator and the resampler on the device (include/adsb_hip.h, "Frequency shift"), held bit for bit to
the numpy restatement of its definition composed with the restated filters (tests/mix_support.py), and its frames to the
reference's and the CPU oracle's.  Shapes are built from t = adsb_*_selftest_tile, the outputs one workgroup takes.  Every
comparison is at tolerance 0."""
import subprocess

import numpy as np
import pytest

from tests import decim_support as ds
from tests import mix_support as ms
from tests import resamp_support as rs
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CHUNK = 131072
CS16, U8 = 0, 1
PERIODS = [1, 2, 3, 4, 7, 25, 125, 256]


def t_soapy() -> np.ndarray:
    x = np.arange(256, dtype=np.float32)
    return np.trunc((x - np.float32(127.4)) * np.float32(1.0 / 128.0) * np.float32(32767.0)).astype(np.int16)


def widen(b: np.ndarray, table: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(table[b.reshape(-1, 2)])


def key(m):
    return (m.chunk, m.j, m.try_phase, m.score, m.msglen, m.msg.hex(), m.signal_level)


def assert_same(msgs, want):
    exp = [(w["chunk"], w["j"], w["try_phase"], w["score"], w["len"], w["msg"].hex(), w["signal_level"]) for w in want]
    assert [key(m) for m in msgs] == exp


@pytest.fixture()
def ctx(hip_lib):
    """A context whose input is ordered behind a torch stream (adsb_set_stream): run() copies in, filters and reads back
    in that stream's order, with no other synchronisation -- set_mixer is ordered on it too."""
    import torch
    from dump1090_rs_amd import Context
    with Context(0, 1) as c:
        c.torch_stream = torch.cuda.Stream()
        c.set_stream(c.torch_stream.cuda_stream)
        yield c
        torch.cuda.synchronize()


def run(h, x: np.ndarray, fmt: int = CS16) -> np.ndarray:
    """One *_run_device call of a decimator or resampler on x ((n, 2) int16, or uint8 for the 8-bit format) -> its
    outputs, (n_out, 2) int16."""
    import torch
    want_n = h.out_count(len(x))
    with torch.cuda.stream(h._ctx.torch_stream):
        d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        d_out = torch.full((max(want_n, 1) + 8, 2), 0x5A5A, dtype=torch.int16, device="cuda")
        n = h.run_device(d_in.data_ptr(), len(x), d_out.data_ptr(), want_n, format=fmt)
        assert n == want_n
        y = d_out.cpu().numpy()
    assert (y[n:] == 0x5A5A).all()   # the canary: nothing written behind the call's outputs
    return y[:n]


class Decim:
    """A decimator by D as a ratio 1 / D: what the tests below need of both kinds under one name."""

    def __init__(self, D):
        self.L, self.M, self.D = 1, D, D

    def tile(self, lib):
        return int(lib.adsb_decim_selftest_tile())

    def taps(self, rng, which):
        T, s = {"one": (1, 0), "default": (8 * self.D + 1, 14), "maximal": (512, 16)}[which]
        return ds.random_taps(rng, T), s, T - 1

    def device(self, ctx, h, s):
        return ctx.decimator(self.D, h, s)

    def restated(self, h, s):
        return ms.DecimStream(h, self.D, s)


class Resamp:
    def __init__(self, L, M):
        self.L, self.M = L, M

    def tile(self, lib):
        return int(lib.adsb_resamp_selftest_tile(self.L, self.M))

    def taps(self, rng, which):
        T, s = {"one": (1, 0), "default": (8 * max(self.L, self.M) + 1, 14), "maximal": (rs.max_taps(self.L), 16)}[which]
        return rs.random_phase_taps(rng, T, self.L), s, rs.phase_taps(self.L, T) - 1

    def device(self, ctx, h, s):
        return ctx.resampler(self.L, self.M, h, s)

    def restated(self, h, s):
        return ms.ResampStream(h, self.L, self.M, s)


def kind_of(L, M, decim=False):
    return Decim(M) if decim else Resamp(L, M)


def inputs_for(L: int, M: int, P: int, count: int) -> int:
    """The fewest inputs behind P consumed ones that give at least `count` outputs: up to the newest input of the last."""
    if count == 0:
        return 0
    last = rs.ceil_div(P * L, M) + count - 1
    return (last * M) // L - P + 1


KINDS = [("decim", 1, 2), ("decim", 1, 16), ("resamp", 1, 1), ("resamp", 6, 5), ("resamp", 3, 25), ("resamp", 24, 125)]


# ----------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("N", PERIODS)
@pytest.mark.parametrize("kind, L, M", KINDS)
def test_exact_against_numpy(hip_lib, ctx, kind, L, M, N):
    k = kind_of(L, M, kind == "decim")
    t = k.tile(hip_lib)
    rng = np.random.default_rng([1, L, M, N])
    w = ms.random_table(rng, N)
    assert np.abs(w.astype(np.int64)).max() == 32767 and w.min() == -32767
    n0 = 2 if N == 3 else 3   # the short first call: the long one starts at a P that is no multiple of N (N > 1)
    wraps = set()
    for which in ("one", "default", "maximal"):
        h, s, H = k.taps(rng, which)
        with k.device(ctx, h, s) as dev:
            dev.set_mixer(w)
            assert dev.mixer_period == N
            for count in (0, 1, t - 1, t, t + 1, 2 * t + 1):
                n_in = inputs_for(L, M, n0, count)
                x = rs.random_iq(rng, n0 + n_in, run=min(H + 1, n_in // 3))
                ref = k.restated(h, s)
                ref.set_mixer(w)
                dev.reset()
                for lo, hi in ((0, n0), (n0, len(x))):
                    got = run(dev, x[lo:hi])
                    assert np.array_equal(got, ref.run(x[lo:hi])), (kind, L, M, N, which, count, lo)
                assert count <= len(got) <= count + (L > M)
                # where the wrap N - 1 -> 0 fell, as sample indices of the long call: inside a 16-byte load group (the
                # call's input is 16-byte aligned: groups of four), and inside what becomes the history
                m = np.arange(n0, len(x))
                at = m[m % N == N - 1] - n0
                wraps |= {"group"} if ((at % 4) != 3).any() else set()
                wraps |= {"history"} if H > 1 and (at >= n_in - H).any() and (at < n_in - 1).any() else set()
    assert wraps == {"group", "history"}


# ----------------------------------------------------------------------------------------------- 2. cut-invariance
@pytest.mark.parametrize("kind, L, M, which, N", [("decim", 1, 2, "default", 7), ("decim", 1, 16, "maximal", 256),
                                                  ("resamp", 6, 5, "default", 25), ("resamp", 3, 25, "maximal", 125),
                                                  ("resamp", 24, 125, "default", 3)])
def test_the_cut_is_invisible(hip_lib, ctx, kind, L, M, which, N):
    k = kind_of(L, M, kind == "decim")
    t = k.tile(hip_lib)
    rng = np.random.default_rng([2, L, M, N])
    h, s, H = k.taps(rng, which)
    w = ms.random_table(rng, N)
    x = rs.random_iq(rng, inputs_for(L, M, 0, 3 * t + 1) + 7, run=H + 1)
    want = ms.decimate(x, h, M, s, w) if kind == "decim" else ms.resample(x, h, L, M, s, w)
    # calls of no input, shorter than the history (the history kernels pass their previous history through), shorter than N
    lengths = sorted({0, 1, 2, N - 1, N, N + 1, H - 1, H, H + 1, t * M // L + 1})
    plan = rs.cut_plan(rng, len(x), lengths, max(L, M))
    assert set(lengths) <= set(plan)
    ref = k.restated(h, s)
    ref.set_mixer(w)
    with k.device(ctx, h, s) as dev:
        dev.set_mixer(w)
        got, at, short, phases = [], 0, 0, set()
        for n in plan:
            phases.add(ref.P % N)
            short += 0 < n < H
            y = run(dev, x[at:at + n])
            assert np.array_equal(y, ref.run(x[at:at + n])), (at, n)
            got.append(y)
            at += n
        assert short > 0 and len(phases) >= min(N, 3)
        assert np.array_equal(np.concatenate(got), want)
        # one call is the same, and after a reset the table starts over with the stream
        dev.reset()
        assert np.array_equal(run(dev, x), want)
        dev.reset()
        assert np.array_equal(np.concatenate([run(dev, x[:H // 2 + 3]), run(dev, x[H // 2 + 3:])]), want)


# ----------------------------------------------------------------------------------------------- 3. rounding, clamping
def test_rounding_and_clamping_at_the_rails(hip_lib, ctx):
    # 1/1 with the tap 1 and shift 0: y[n] = x'[n], the mixer's output itself
    with ctx.resampler(1, 1, [1], 0) as res:
        def mixed(x, w):
            res.reset()
            res.set_mixer(np.array(w, np.int16).reshape(-1, 2))
            x = np.array(x, np.int16).reshape(-1, 2)
            got = run(res, x)
            assert np.array_equal(got, ms.mix(x, w))
            return got.tolist()
        assert mixed([[1, 0], [-1, 0], [0, 1], [0, -1]], [[8192, 0]]) == [[1, 0], [0, 0], [0, 1], [0, 0]]   # a half rounds up
        assert mixed([[32767, 32767], [32767, -32767], [-32767, -32767]], [[23170, 23170]]) == [[0, 32767], [32767, 0], [0, -32768]]
        rails = [[-32768, 32767]] * 4 + [[32767, -32768]] * 4 + [[-32768, -32768]] * 4
        corners = [[32767, 32767], [32767, -32767], [-32767, 32767], [-32767, -32767]]
        got = mixed(rails, corners)
        # (-+65535 x 32767 + 8192) >> 14 clamps; the other half is (-32767 + 8192) >> 14
        assert got[0] == [-32768, -2] and got[1] == [-2, 32767]
        assert all({-32768, 32767} <= {g[half] for g in got} for half in (0, 1))
    # x'[m < 0] = 0: the first outputs see nothing in front of the stream, also where the 8-bit table's T8[0] is not zero
    table = rs.rail_u8_table()
    w = ms.random_table(np.random.default_rng(3), 7)
    ctx.set_u8_table(table)
    try:
        with ctx.decimator(2, [1, 1, 1], 0) as dec:
            dec.set_mixer(w)
            b = np.zeros((9, 2), np.uint8)
            xm = ms.mix(widen(b, table), w).astype(np.int64)
            assert table[0] == -32768 and xm[0].tolist() != [0, 0]
            want = np.clip(np.array([xm[0], xm[0] + xm[1] + xm[2], xm[2] + xm[3] + xm[4], xm[4] + xm[5] + xm[6], xm[6] + xm[7] + xm[8]]),
                           -32768, 32767)
            assert np.array_equal(run(dec, b, U8), want)
    finally:
        import torch
        torch.cuda.synchronize()
        ctx.set_u8_table(None)


# ----------------------------------------------------------------------------------------------- 4. 8-bit
@pytest.mark.parametrize("kind, L, M, N", [("decim", 1, 5, 25), ("resamp", 6, 5, 7), ("resamp", 3, 10, 256)])
@pytest.mark.parametrize("table_name", ["soapy", "rails"])
def test_8bit_input_is_widened_then_mixed(hip_lib, ctx, kind, L, M, N, table_name):
    import torch
    k = kind_of(L, M, kind == "decim")
    t = k.tile(hip_lib)
    rng = np.random.default_rng([4, L, M])
    h, s, H = k.taps(rng, "default")
    w = ms.random_table(rng, N)
    table = t_soapy() if table_name == "soapy" else rs.rail_u8_table()
    b = rng.integers(0, 256, size=(inputs_for(L, M, 0, t + 3) + 2, 2), dtype=np.uint8)
    b[: H + 5] = 0   # bytes 0 at the start: T8[0] behind the stream's start, zeros in front of it
    xw = widen(b, table)
    want = ms.decimate(xw, h, M, s, w) if kind == "decim" else ms.resample(xw, h, L, M, s, w)
    ctx.set_u8_table(table)
    try:
        with k.device(ctx, h, s) as dev:
            dev.set_mixer(w)
            assert np.array_equal(run(dev, b, U8), want)
            # a stream that alternates CS16 calls and 8-bit calls of the same widened samples
            dev.reset()
            cuts = [0, 1, H // 2 + 1, H + M, len(b) // 2, len(b)]
            parts = [run(dev, b[lo:hi], U8) if i % 2 else run(dev, xw[lo:hi]) for i, (lo, hi) in enumerate(zip(cuts, cuts[1:]))]
            assert np.array_equal(np.concatenate(parts), want)
    finally:
        torch.cuda.synchronize()
        ctx.set_u8_table(None)


# ----------------------------------------------------------------------------------------------- 5. set, change, clear
@pytest.mark.parametrize("kind, L, M", [("decim", 1, 5), ("resamp", 6, 25)])
def test_set_change_and_clear_between_calls(hip_lib, ctx, kind, L, M):
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd._lib import AdsbError
    k = kind_of(L, M, kind == "decim")
    t = k.tile(hip_lib)
    rng = np.random.default_rng([5, L, M])
    h, s, H = k.taps(rng, "default")
    x = rs.random_iq(rng, inputs_for(L, M, 0, 2 * t + 5), run=H)
    w7, w256, w4 = ms.random_table(rng, 7), ms.random_table(rng, 256), ms.rotation(1)
    # the schedule: calls shorter than the history among them, so that mixed, differently mixed and plain samples meet in it
    cuts = [0, 5, 5 + H // 2, 5 + H, len(x) // 3, len(x) // 3 + 2, len(x) // 2, len(x)]
    tabs = [None, w7, w7, w256, None, w4, w256]
    ref = k.restated(h, s)
    set_mixer = hip_lib.adsb_mix_set_decim if kind == "decim" else hip_lib.adsb_mix_set_resamp
    with k.device(ctx, h, s) as dev, k.device(ctx, h, s) as plain:
        assert dev.mixer_period == 0
        got, never = [], []
        for (lo, hi), tab in zip(zip(cuts, cuts[1:]), tabs):
            dev.set_mixer(tab)
            ref.set_mixer(tab)
            assert dev.mixer_period == (0 if tab is None else len(tab))
            # an invalid table is refused and changes nothing: -32768 in it, too long, no table, a table of no length
            bad = np.array(w7)
            bad[6, 1] = -32768
            for ptr, n in ((bad.ctypes.data, 7), (w256.ctypes.data, 257), (None, 3), (w7.ctypes.data, 0)):
                assert set_mixer(dev._h, ptr, n) == _lib.ADSB_ERR_INVALID
            assert dev.mixer_period == (0 if tab is None else len(tab))
            y = run(dev, x[lo:hi])
            assert np.array_equal(y, ref.run(x[lo:hi])), (lo, hi)
            got.append(y)
            never.append(run(plain, x[lo:hi]))
        with pytest.raises(AdsbError):
            dev.set_mixer(np.full((3, 2), -32768, np.int16))
        with pytest.raises(ValueError):
            dev.set_mixer(np.zeros(6, np.int16))
        # mixer off is byte-equal to a handle that never had one: a stream of its own, after a mixer was set and cleared
        dev.reset()
        plain.reset()
        dev.set_mixer(w7)
        dev.set_mixer(None)
        a, b = run(dev, x), run(plain, x)
        assert a.tobytes() == b.tobytes() and np.array_equal(b, (ds.decimate(x, h, M, s) if kind == "decim" else rs.resample(x, h, L, M, s)))
        assert not np.array_equal(np.concatenate(got), np.concatenate(never))


# ----------------------------------------------------------------------------------------------- 6. frames, pinned
@pytest.mark.parametrize("kind, L, M", [("resamp", 2, 5), ("resamp", 24, 25), ("decim", 1, 4)])
def test_rotated_held_golden_captures_give_the_reference_frames(hip_lib, golden, fixture_iq, kind, L, M):
    import torch
    from dump1090_rs_amd import Context, mixer_table
    k = kind_of(L, M, kind == "decim")
    rng = np.random.default_rng([6, L, M])
    back = mixer_table(3, 4)
    assert np.array_equal(back, ms.rotation(3))
    with Context(0, 1) as c, k.device(c, [1] * L, 0) as dev:
        dev.set_mixer(back)
        for fx in golden["fixtures"]:
            cap = fixture_iq[fx["file"]]
            assert cap.min() > -32768   # (then the rotation by j^m is exact)
            x = np.maximum(rs.hold_input(cap, L, M, rng), -32767)   # x[floor(n M / L)] = capture[n], random elsewhere
            tuned = ms.mix(x, ms.rotation(1))                        # ... as an offset-tuned radio delivers it: x[m] j^m
            assert np.array_equal(ms.mix(tuned, back), x) and np.array_equal(rs.resample(x, [1] * L, L, M, 0), cap)
            c.icao_flush()
            dev.reset()
            got = dev.demod_iq(tuned)
            assert [m.buffer().hex() for m in got] == fx["frames"] and len(got) in (5, 6)
            assert [m.j for m in got] == fx["j"] and [m.try_phase for m in got] == fx["try_phase"]
            # run_device + submit + collect, nothing in between: the pass waits for the filter by itself
            d_in = torch.from_numpy(tuned).cuda()
            d_out = torch.empty((CHUNK, 2), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            c.icao_flush()
            dev.reset()
            n = dev.run_device(d_in.data_ptr(), len(tuned), d_out.data_ptr(), CHUNK)
            c.submit_iq_device(d_out.data_ptr(), n)
            again = c.collect()
            assert n == CHUNK and [key(m) for m in again] == [key(m) for m in got]


# ----------------------------------------------------------------------------------------------- 7. a real filter
@pytest.mark.parametrize("D, kk, N", [(4, 1, 4), (5, 6, 25), (10, 3, 25)])
def test_offset_tuned_captures_through_the_default_filter_match_the_oracle(hip_lib, oracle_mod, golden, fixture_iq, D, kk, N):
    """Each capture as a radio at D x 2.4 MS/s tuned k / N of its rate beside 1090 MHz would have delivered it -- the
    capture interpolated by D and shifted, both in numpy -- brought back by the device's counter-shift and default filter:
    equal to the oracle on the restatement.  The shares of the reference's frames that come back, plain and with a DC
    offset of 1000 added at the high rate, are printed, not asserted."""
    from dump1090_rs_amd import Context, mixer_for_shift, mixer_table
    h = ds.hamming_sinc_taps(D)   # numpy's table of the default taps' formula: the expectation does not hang on libm
    assert mixer_for_shift(1, D, -(2_400_000 * D * kk // N)) == (N - kk, N)
    w = mixer_table(N - kk, N)
    assert np.abs(w.astype(np.int64) - ms.table(N - kk, N)).max() <= 1
    orc = oracle_mod.Oracle()
    total = found = found_dc = n_ref = 0
    with Context(0, 1) as c, c.decimator(D, h, 15) as dec:
        dec.set_mixer(w)
        for fx in golden["fixtures"]:
            up = rs.resample(fixture_iq[fx["file"]], rs.hamming_sinc_taps(D, 1), D, 1, 14)
            x = ms.shift_spectrum(up, kk, N)
            orc.icao_flush()
            want, _ = orc.demod_iq(ms.decimate(x, h, D, 15, w))
            total += len(want)
            found += len(set(f["buffer"].hex() for f in want) & set(fx["frames"]))
            n_ref += len(fx["frames"])
            c.icao_flush()
            dec.reset()
            assert_same(dec.demod_iq(x), want)
            dc = np.clip(x.astype(np.int64) + 1000, -32768, 32767).astype(np.int16)
            orc.icao_flush()
            found_dc += len(set(f["buffer"].hex() for f in orc.demod_iq(ms.decimate(dc, h, D, 15, w))[0]) & set(fx["frames"]))
    print(f"D = {D}, shift {kk}/{N}: {found} of the reference's {n_ref} frames; with DC 1000 added: {found_dc}")
    assert total >= 1   # (a precondition, not a tolerance: the comparison is not empty)


# ----------------------------------------------------------------------------------------------- 8. adsb_feed
def test_adsb_feed_decimate_shift(hip_lib, oracle_mod, golden, fixture_iq, tmp_path):
    from dump1090_rs_amd import default_taps, mixer_table
    D = 4
    fx = golden["fixtures"][2]
    # a radio at 9.6 MS/s tuned 2.4 MHz below 1090 MHz: the signal a quarter of the rate above its centre, x[m] j^m
    x = ms.mix(np.repeat(fixture_iq[fx["file"]], D, axis=0), ms.rotation(1))
    path = tmp_path / "x4_offset.iq"
    np.ascontiguousarray(x[:, ::-1]).astype("<i2").tofile(path)   # the capture format: im first
    h, s = default_taps(D)
    want, _ = oracle_mod.Oracle().demod_iq(ms.decimate(x, h, D, s, mixer_table(3, 4)))
    assert len(want) > 0
    feed = str(ROOT / "dump1090_rs_amd" / "adsb_feed")
    r = subprocess.run([feed, "--decimate", str(D), "--shift", "-2400000", "--buffers", "2", str(path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["*" + w["buffer"].hex() + ";" for w in want]
    # without the counter-shift the decimator's low-pass removes the signal with everything else beside its band
    plain = subprocess.run([feed, "--decimate", str(D), "--buffers", "2", str(path)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.splitlines() != r.stdout.splitlines()
