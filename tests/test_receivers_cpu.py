"""Many receivers, one pass -- the host side, without a GPU: adsb_replay_records_rx (the ordered replay with one ICAO
filter per receiver, serially and with the receivers dealt to several threads) against one CPU oracle per receiver on the
oracle's own trial records, the argument checks of every _rx entry point, and the replay under the address / undefined-
behaviour and thread sanitizers in a stand-alone program (tests/receivers_replay_san.cpp)."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import receivers_support as RS
from tests.conftest import ROOT

SRC = ROOT / "dump1090_rs_amd" / "csrc" / "adsb_replay_host.cpp"
PER = 3   # buffers per receiver


def replay_rx(records, m, n_receivers, mode=0, threads=1, tables=None):
    from dump1090_rs_amd import context
    tables = np.zeros((n_receivers, 4096), dtype=np.uint32) if tables is None else tables
    msgs = context.replay_records_rx(records, m, tables, mode=mode, threads=threads, cap=1 << 17)
    return RS.keys(msgs), tables


@pytest.fixture(scope="module")
def records_of():
    """{(receivers, fix): the oracle's trial records of RS.batch(receivers, PER)} -- computed once, never changed"""
    cache = {}

    def get(n, fix=False):
        if (n, fix) not in cache:
            rec = RS.trial_records(RS.batch(n, PER, fix=fix)[0])
            rec.setflags(write=False)
            cache[(n, fix)] = rec
        return cache[(n, fix)]
    return get


@pytest.mark.parametrize("n_receivers", [1, 2, 3, 7])
def test_serial_replay_equals_one_oracle_per_receiver(hip_lib, oracle_mod, records_of, n_receivers):
    iq, m = RS.batch(n_receivers, PER)
    want, shared, model = RS.expectations(n_receivers, PER)
    RS.assert_tells_apart(n_receivers, want, shared)
    assert len(want) > 100 * n_receivers
    got, tables = replay_rx(records_of(n_receivers), m, n_receivers)
    assert got == want
    for r in range(n_receivers):
        assert list(tables[r]) == model.table(r), r
    # the records in any order
    rec = records_of(n_receivers).copy()
    np.random.default_rng(n_receivers).shuffle(rec)
    got2, tables2 = replay_rx(rec, m, n_receivers)
    assert got2 == want and np.array_equal(tables2, tables)


def test_one_receiver_is_the_plain_replay_byte_for_byte(hip_lib, oracle_mod, records_of):
    from dump1090_rs_amd._lib import AdsbMsg
    rec = records_of(1)
    m = np.zeros(PER, dtype=np.uint32)
    for mode in (0, 1, 3):
        out = [(AdsbMsg * (1 << 16))(), (AdsbMsg * (1 << 16))()]
        tab = [np.zeros(4096, dtype=np.uint32), np.zeros(4096, dtype=np.uint32)]
        n = [C.c_size_t(), C.c_size_t()]
        a, b = rec.copy(), rec.copy()
        assert hip_lib.adsb_replay_records_fix(tab[0].ctypes.data, a.ctypes.data, len(a), mode, out[0], 1 << 16, C.byref(n[0])) == 0
        assert hip_lib.adsb_replay_records_rx(tab[1].ctypes.data, 1, m.ctypes.data, PER, b.ctypes.data, len(b), mode, 1, out[1],
                                              1 << 16, C.byref(n[1])) == 0
        assert n[0].value == n[1].value > 100
        size = n[0].value * C.sizeof(AdsbMsg)
        assert C.string_at(out[0], size) == C.string_at(out[1], size)
        assert np.array_equal(tab[0], tab[1]) and np.array_equal(a, b)


@pytest.mark.parametrize("n_receivers", [2, 3, 7])
@pytest.mark.parametrize("threads", [2, 3, 7])
def test_threads_equal_serial(hip_lib, oracle_mod, records_of, n_receivers, threads):
    m = RS.batch(n_receivers, PER)[1]
    want, tables = replay_rx(records_of(n_receivers), m, n_receivers)
    got, tables_t = replay_rx(records_of(n_receivers), m, n_receivers, threads=threads)
    assert got == want and len(want) > 100 * n_receivers
    assert np.array_equal(tables_t, tables)
    # ... and from filters that hold something already: the same input a second time
    want2, _ = replay_rx(records_of(n_receivers), m, n_receivers, tables=tables)
    got2, _ = replay_rx(records_of(n_receivers), m, n_receivers, threads=threads, tables=tables_t)
    assert got2 == want2 and got2 != want and np.array_equal(tables_t, tables)


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_error_correction_modes(hip_lib, oracle_mod, records_of, mode):
    """ADSB_FIX_NONE / 1BIT / 2BIT on a capture with damaged DF17 / DF18 copies: a repair consults the filter of the
    trial's own receiver.  Against one restatement of the mode per receiver."""
    n_receivers = 3
    iq, m = RS.batch(n_receivers, PER, fix=True)
    want, shared, model = RS.expectations(n_receivers, PER, fix=True, mode=mode)
    RS.assert_tells_apart(n_receivers, want, shared)
    if mode:
        assert sum(k[3] == 1200 for k in want) >= 10 * n_receivers
    for threads in (1, 3):
        got, tables = replay_rx(records_of(n_receivers, True), m, n_receivers, mode=mode, threads=threads)
        assert got == want, threads
        for r in range(n_receivers):
            assert list(tables[r]) == model.table(r), r


def test_capacity_and_bad_arguments(hip_lib, oracle_mod, records_of):
    from dump1090_rs_amd._lib import AdsbMsg
    L = hip_lib
    n_receivers = 2
    rec, m = records_of(n_receivers).copy(), RS.batch(n_receivers, PER)[1].copy()
    want, _ = replay_rx(rec, m, n_receivers)

    def call(tables, n_rx, mp, n_buf, r, n_rec, mode=0, threads=1, cap=1 << 16):
        out, n = (AdsbMsg * max(cap, 1))(), C.c_size_t()
        st = L.adsb_replay_records_rx(None if tables is None else tables.ctypes.data, n_rx, None if mp is None else mp.ctypes.data,
                                      n_buf, None if r is None else r.ctypes.data, n_rec, mode, threads, out if cap else None, cap,
                                      C.byref(n))
        return st, n.value, out

    tables = np.zeros((n_receivers, 4096), dtype=np.uint32)
    st, n, out = call(tables, n_receivers, m, len(m), rec, len(rec), cap=5)
    assert st == -5 and n == len(want)                                    # ADSB_ERR_CAPACITY with the full count
    assert [(o.chunk, o.j) for o in out[:5]] == [k[:2] for k in want[:5]]
    clean = np.zeros((n_receivers, 4096), dtype=np.uint32)
    for bad in (lambda: call(None, n_receivers, m, len(m), rec, len(rec)),          # null pointers
                lambda: call(clean, n_receivers, None, len(m), rec, len(rec)),
                lambda: call(clean, n_receivers, m, len(m), None, len(rec)),
                lambda: call(clean, 0, m, len(m), rec, len(rec)),                     # no receivers
                lambda: call(clean, 16385, m, len(m), rec, len(rec)),                 # more than ADSB_MAX_RECEIVERS
                lambda: call(clean, n_receivers, m, len(m), rec, len(rec), mode=2),   # no such mode
                lambda: call(clean, 1, m, len(m), rec, len(rec)),                     # map entry out of range
                lambda: call(clean, n_receivers, m, len(m) - 1, rec, len(rec))):      # a record's buffer outside the map
        assert bad()[0] == -1
        assert not clean.any()                                             # ... and no table touched
    out, n = (AdsbMsg * 4)(), C.c_size_t()
    assert L.adsb_replay_records_rx(clean.ctypes.data, n_receivers, m.ctypes.data, len(m), rec.ctypes.data, len(rec), 0, 1, None, 4,
                                    C.byref(n)) == -1
    assert L.adsb_replay_records_rx(clean.ctypes.data, n_receivers, None, 0, None, 0, 0, 1, None, 0, C.byref(n)) == 0 and n.value == 0


def test_rx_entry_points_refuse_a_null_context_without_a_device(hip_lib):
    L = hip_lib
    m = (C.c_uint32 * 4)()
    iq = (C.c_int16 * 8)()
    n = C.c_size_t()
    assert L.adsb_set_receivers(None, 2) == -1 and L.adsb_get_receivers(None) == -1
    assert L.adsb_icao_flush_receiver(None, 0) == -1
    assert L.adsb_receiver_filter_table(None, 0, (C.c_uint32 * 4096)()) == -1
    for name in ("adsb_demod_iq_rx", "adsb_demod_iq_device_rx", "adsb_demod_iq_rx_u8", "adsb_demod_iq_device_rx_u8"):
        assert getattr(L, name)(None, iq, 4, m, None, 0, C.byref(n)) == -1, name
    assert L.adsb_submit_iq_device_rx(None, iq, 4, m) == -1 and L.adsb_submit_iq_device_rx_u8(None, iq, 4, m) == -1
    assert L.adsb_ring_submit_rx(None, 4, m) == -1
    assert L.adsb_selftest_rx_tune(None, 0) == -1 and L.adsb_selftest_rx_counters(None, (C.c_uint64 * 4)()) == -1


def _sanitized(flag: str, runtime: str) -> subprocess.CompletedProcess:
    lib = subprocess.run(["gcc", f"-print-file-name={runtime}"], capture_output=True, text=True).stdout.strip()
    if not lib or not Path(lib).exists() or shutil.which("g++") is None:
        pytest.skip(f"no {runtime} / g++ in this environment")
    exe = ROOT / "tests" / ("receivers_replay_" + ("tsan" if "thread" in flag else "asan"))
    src = [ROOT / "tests" / "receivers_replay_san.cpp", SRC]
    hdrs = [SRC.parent / n for n in ("adsb_replay_host.h", "adsb_record.h", "mode_s_host.hpp")] + [ROOT / "include" / "adsb_hip.h"]
    if not exe.exists() or exe.stat().st_mtime < max(p.stat().st_mtime for p in [*src, *hdrs]):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", flag, "-fno-omit-frame-pointer", "-pthread",
                        *map(str, src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe), "120"], capture_output=True, text=True, timeout=600,
                          env=dict(__import__("os").environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1",
                                   UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_receiver_replay_under_address_and_ub_sanitizers():
    """tests/receivers_replay_san.cpp, a program of its own (nothing loaded into python): seeded random record sets
    replayed serially and through the pool -- filters carried across captures, per-receiver flushes, a receiver that
    fills its 4096-slot table -- same messages, same tables, no report."""
    r = _sanitized("-fsanitize=address,undefined", "libasan.so")
    assert r.returncode == 0 and "receiver replay ok: 120 captures" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_receiver_replay_under_thread_sanitizer():
    r = _sanitized("-fsanitize=thread", "libtsan.so")
    if "unexpected memory mapping" in r.stderr:   # (a kernel whose address-space layout this libtsan does not know)
        pytest.skip("ThreadSanitizer cannot run on this kernel")
    assert r.returncode == 0 and "receiver replay ok: 120 captures" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
