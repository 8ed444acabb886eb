"""The decimator on the device (include/adsb_hip.h, "Decimation"), held bit for bit to the numpy restatement of its
definition (tests/decim_support.py), and its frames to the reference's and the CPU oracle's.  Shapes: the smallest at
which the kernel can go wrong -- around one and two tiles of outputs, every residue of P mod D at a cut, calls shorter
than the history."""
import subprocess

import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import decim_support as ds
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CHUNK = 131072
CS16, U8 = 0, 1


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
    """A context whose input is ordered behind a torch stream (adsb_set_stream): run() copies in, decimates and reads back
    in that stream's order, with no other synchronisation."""
    import torch
    from dump1090_rs_amd import Context
    with Context(0, 1) as c:
        c.torch_stream = torch.cuda.Stream()
        c.set_stream(c.torch_stream.cuda_stream)
        yield c
        torch.cuda.synchronize()


def tile(hip_lib) -> int:
    return int(hip_lib.adsb_decim_selftest_tile())


def run(dec, x: np.ndarray, fmt: int = CS16, cap=None) -> np.ndarray:
    """One adsb_decim_run_device call on x ((n, 2) int16, or uint8 for the 8-bit format) -> its outputs, (n_out, 2) int16."""
    import torch
    want_n = dec.out_count(len(x))
    cap = want_n if cap is None else cap
    with torch.cuda.stream(dec._ctx.torch_stream):
        d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        d_out = torch.full((max(cap, 1) + 8, 2), 0x5A5A, dtype=torch.int16, device="cuda")
        n = dec.run_device(d_in.data_ptr(), len(x), d_out.data_ptr(), cap, format=fmt)
        assert n == want_n
        y = d_out.cpu().numpy()
    assert (y[n:] == 0x5A5A).all()   # nothing written behind the call's outputs
    return y[:n]


def n_in_for(count: int, D: int) -> int:
    """An input length, no multiple of D, that gives `count` outputs from the start of a stream."""
    return 0 if count == 0 else (count - 1) * D + (1 if D == 2 else 2)


# ----------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("D", [2, 3, 5, 16])
def test_exact_against_numpy(hip_lib, ctx, D):
    t = tile(hip_lib)
    rng = np.random.default_rng(1000 + D)
    for T in sorted({1, 2, D, 8 * D + 1, 512}):
        h = ds.random_taps(rng, T)   # sum |h| = 65534 (T = 1: 32767, all one tap can hold)
        for s in (0, 1, 15, 16):
            with ctx.decimator(D, h, s) as dec:
                for count in (0, 1, t - 1, t, t + 1, 2 * t + 1):
                    n_in = n_in_for(count, D)
                    assert n_in % D or n_in == 0
                    x = ds.random_iq(rng, n_in, run=min(T, n_in // 3))
                    dec.reset()
                    got = run(dec, x)
                    assert len(got) == count
                    assert np.array_equal(got, ds.decimate(x, h, D, s)), (D, T, s, count)
                # no output at all from a call that has input: one input, then D - 1 that reach no output, then the rest
                x = ds.random_iq(rng, n_in_for(t + 1, D), run=min(T, 50))
                dec.reset()
                parts = [run(dec, x[:1]), run(dec, x[1:D]), run(dec, x[D:])]
                assert [len(p) for p in parts] == [1, 0, t]
                assert np.array_equal(np.concatenate(parts), ds.decimate(x, h, D, s)), (D, T, s)


# ----------------------------------------------------------------------------------------------- 2. rounding, clamping
def test_rounding_and_clamping(hip_lib, ctx):
    with ctx.decimator(2, [1], 1) as dec:
        x = np.repeat(np.array([[-3, 3], [-1, 1], [1, -1], [3, -3]], np.int16), 2, axis=0)
        assert run(dec, x).tolist() == [[-1, 2], [0, 1], [1, 0], [2, -1]]   # a half rounds up
    with ctx.decimator(2, [32767, 32767], 0) as dec:
        x = np.array([[-32768, 32767]] * 6 + [[32767, -32768]] * 6, np.int16)
        got = run(dec, x)
        assert got[1:3].tolist() == [[-32768, 32767]] * 2 and got[4:].tolist() == [[32767, -32768]] * 2
        assert np.array_equal(got, ds.decimate(x, [32767, 32767], 2, 0))


# ----------------------------------------------------------------------------------------------- 3. cut-invariance
@pytest.mark.parametrize("D, T, s", [(2, 17, 15), (3, 2, 1), (5, 41, 15), (16, 1, 0), (16, 129, 15), (16, 512, 16)])
def test_the_cut_is_invisible(hip_lib, ctx, D, T, s):
    t = tile(hip_lib)
    rng = np.random.default_rng(2000 + 16 * T + D)
    h = ds.random_taps(rng, T)
    x = ds.random_iq(rng, 3 * t * D + 7, run=T)
    want = ds.decimate(x, h, D, s)
    lengths = sorted({0, 1, D - 1, D, D + 1, max(T - 2, 0), T - 1, T, t * D + 1})
    plan = ds.cut_plan(rng, len(x), lengths, D)
    assert set(lengths) <= set(plan)
    ref = ds.Stream(h, D, s)
    with ctx.decimator(D, h, s) as dec:
        got, at, residues = [], 0, set()
        for n in plan:
            residues.add(ref.P % D)
            assert dec.out_count(n) == ref.out_count(n)
            y = run(dec, x[at:at + n])
            assert np.array_equal(y, ref.run(x[at:at + n])), (at, n)
            got.append(y)
            at += n
        assert residues == set(range(D))
        assert np.array_equal(np.concatenate(got), want)
        # and one call is the same; after reset the same stream gives the same outputs again
        dec.reset()
        assert np.array_equal(run(dec, x), want)
        dec.reset()
        assert np.array_equal(np.concatenate([run(dec, x[:T // 2 + 3]), run(dec, x[T // 2 + 3:])]), want)


# ----------------------------------------------------------------------------------------------- 4. 8-bit
@pytest.mark.parametrize("D, T", [(2, 17), (5, 512), (16, 3)])
def test_8bit_input(hip_lib, ctx, D, T):
    t = tile(hip_lib)
    rng = np.random.default_rng(3000 + D)
    h, s = ds.random_taps(rng, T), 15
    table = t_soapy()
    assert table[0] != 0
    b = rng.integers(0, 256, size=(t * D + D + 3, 2), dtype=np.uint8)
    b[: T + 5] = 0   # bytes 0 at the start: T8[0] behind the stream's start, zeros in front of it
    want = ds.decimate(widen(b, table), h, D, s)
    # (a history of T8[0] in front of the stream would give something else, so the comparison can tell)
    other = ds.Stream(h, D, s)
    other.hist[:] = table[0]
    assert not np.array_equal(other.run(widen(b, table)), want)
    with ctx.decimator(D, h, s) as dec:
        assert np.array_equal(run(dec, b, U8), want)
        dec.reset()
        assert np.array_equal(run(dec, b, U8), want)
        # a stream that alternates CS16 calls and 8-bit calls of the same widened samples
        dec.reset()
        cuts = [0, 1, T // 2 + 1, T + D, len(b) // 2, len(b)]
        parts = []
        for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            parts.append(run(dec, b[lo:hi], U8) if i % 2 else run(dec, widen(b[lo:hi], table)))
        assert np.array_equal(np.concatenate(parts), want)
        # a HackRF's CS8 through a table of the caller's
        cs8 = (np.arange(256).astype(np.uint8).view(np.int8).astype(np.int16) << 8).astype(np.int16)
        ctx.set_u8_table(cs8)
        try:
            dec.reset()
            assert np.array_equal(run(dec, b, U8), ds.decimate(widen(b, cs8), h, D, s))
        finally:
            import torch
            torch.cuda.synchronize()
            ctx.set_u8_table(None)


# ----------------------------------------------------------------------------------------------- 5. capacity
def test_capacity_consumes_nothing(hip_lib, ctx):
    from dump1090_rs_amd import _lib
    from dump1090_rs_amd._lib import AdsbError
    t = tile(hip_lib)
    rng = np.random.default_rng(5)
    D, T, s = 3, 25, 15
    h = ds.random_taps(rng, T)
    x = ds.random_iq(rng, (t + 5) * D + 1, run=T)
    want = ds.decimate(x, h, D, s)
    with ctx.decimator(D, h, s) as dec:
        first = run(dec, x[:100])
        n = dec.out_count(len(x) - 100)
        with pytest.raises(AdsbError) as e:
            run(dec, x[100:], cap=n - 1)
        assert e.value.status == _lib.ADSB_ERR_CAPACITY and e.value.required == n
        assert dec.out_count(len(x) - 100) == n
        assert np.array_equal(np.concatenate([first, run(dec, x[100:])]), want)


# ----------------------------------------------------------------------------------------------- 6. frames, pinned
@pytest.mark.parametrize("D", [2, 5, 16])
def test_repeated_golden_captures_give_the_reference_frames(hip_lib, golden, fixture_iq, D):
    import torch
    from dump1090_rs_amd import Context
    with Context(0, 1) as c, c.decimator(D, [1], 0) as dec:
        for fx in golden["fixtures"]:
            x = np.repeat(fixture_iq[fx["file"]], D, axis=0)
            c.icao_flush()
            dec.reset()
            got = dec.demod_iq(x)
            assert [m.buffer().hex() for m in got] == fx["frames"] and len(got) in (5, 6)
            assert [m.j for m in got] == fx["j"] and [m.try_phase for m in got] == fx["try_phase"]
            # run_device + submit + collect, nothing in between: the pass waits for the decimator by itself
            d_in = torch.from_numpy(x).cuda()
            d_out = torch.empty((CHUNK, 2), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            c.icao_flush()
            dec.reset()
            n = dec.run_device(d_in.data_ptr(), len(x), d_out.data_ptr(), CHUNK)
            c.submit_iq_device(d_out.data_ptr(), n)
            again = c.collect()
            assert n == CHUNK and [key(m) for m in again] == [key(m) for m in got]


# ----------------------------------------------------------------------------------------------- 7. a real filter
@pytest.mark.parametrize("D", [2, 5, 10])
def test_golden_captures_through_the_default_filter_match_the_oracle(hip_lib, oracle_mod, golden, fixture_iq, D):
    from dump1090_rs_amd import Context, default_taps
    h = ds.hamming_sinc_taps(D)   # numpy's table of the default taps' formula: the expectation does not hang on libm
    lib_taps, shift = default_taps(D)
    assert shift == 15 and len(lib_taps) == len(h)
    orc = oracle_mod.Oracle()
    with Context(0, 1) as c, c.decimator(D, h, 15) as dec:
        for fx in golden["fixtures"]:
            x = np.repeat(fixture_iq[fx["file"]], D, axis=0)
            orc.icao_flush()
            want, _ = orc.demod_iq(ds.decimate(x, h, D, 15))
            assert len(want) > 0
            c.icao_flush()
            dec.reset()
            assert_same(dec.demod_iq(x), want)


# ----------------------------------------------------------------------------------------------- 8. a stream of calls
@pytest.mark.parametrize("D, max_chunks, fmt", [(2, 2, CS16), (5, 1, CS16), (3, 16, U8)])
def test_a_stream_over_several_demod_calls(hip_lib, oracle_mod, D, max_chunks, fmt):
    from dump1090_rs_amd import Context
    h, s = np.full(D, 65534 // D, np.int16), 16   # a boxcar over the D copies of a sample
    two_pieces = 2 * CHUNK * D + 1                # two internal pieces on a max_chunks = 2 context at D = 2
    cuts = [100_001, two_pieces, 3, 77_777 * D] if D == 2 else [50_001, CHUNK * D + 12_345, 0, 29_999]
    base = synth.make_iq(-(-sum(cuts) // D), n_bursts=400, seed=800 + D, n_icao=20, df11_every=3)
    if fmt == U8:
        table = t_soapy()
        raw = np.ascontiguousarray(np.clip(np.rint(base / 256.0 + 127.4), 0, 255).astype(np.uint8))
        x, xw = np.repeat(raw, D, axis=0)[: sum(cuts)], np.repeat(widen(raw, table), D, axis=0)[: sum(cuts)]
    else:
        x = xw = np.repeat(base, D, axis=0)[: sum(cuts)]
    orc, ref = oracle_mod.Oracle(), ds.Stream(h, D, s)
    total = 0
    with Context(0, max_chunks) as c, c.decimator(D, h, s) as dec:
        c.icao_flush()
        at = 0
        for n in cuts:
            want, _ = orc.demod_iq(ref.run(xw[at:at + n]), cap=1 << 16)
            assert_same(dec.demod_iq(x[at:at + n], format=fmt, cap=1 << 16), want)
            total += len(want)
            at += n
    assert total > 50


# ----------------------------------------------------------------------------------------------- 9. adsb_feed
def test_adsb_feed_decimate(hip_lib, oracle_mod, golden, fixture_iq, tmp_path):
    from dump1090_rs_amd import default_taps
    D = 5
    fx = golden["fixtures"][2]
    x = np.repeat(fixture_iq[fx["file"]], D, axis=0)
    path = tmp_path / "x5.iq"
    np.ascontiguousarray(x[:, ::-1]).astype("<i2").tofile(path)   # the capture format: im first
    h, s = default_taps(D)
    want, _ = oracle_mod.Oracle().demod_iq(ds.decimate(x, h, D, s))
    assert len(want) > 0
    r = subprocess.run([str(ROOT / "dump1090_rs_amd" / "adsb_feed"), "--decimate", str(D), "--buffers", "2", str(path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["*" + w["buffer"].hex() + ";" for w in want]
