"""Context: one GPU stream of the demod_2400 path (wraps adsb_ctx of include/adsb_hip.h)."""
from __future__ import annotations

import ctypes as C
import struct
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import AdsbError, AdsbMsg, AdsbStats

# reference src/lib.rs:22-26
MODES_MAG_BUF_SAMPLES = 131_072
TRAILING_SAMPLES = 326
MODES_LONG_MSG_BYTES = 14
MODES_SHORT_MSG_BYTES = 7
MAG_DATA_LEN = TRAILING_SAMPLES + MODES_MAG_BUF_SAMPLES
RX_ALL = 0xFFFFFFFF   # ADSB_RX_ALL: every receiver (Context.receiver_carry_reset)


@dataclass
class MagnitudeBuffer:
    """reference src/lib.rs:30-51: 326 zero lead-in samples, then `length` magnitudes."""
    data: np.ndarray = field(default_factory=lambda: np.zeros(MAG_DATA_LEN, dtype=np.uint16))
    length: int = 0
    first_sample_timestamp_12mhz: int = 0

    def push(self, x: int) -> None:  # src/lib.rs:47-50
        if self.length >= MODES_MAG_BUF_SAMPLES:
            raise IndexError("MagnitudeBuffer is full")  # the reference panics (index OOB)
        self.data[TRAILING_SAMPLES + self.length] = x
        self.length += 1


@dataclass(frozen=True)
class ModeSMessage:
    """reference src/demod_2400.rs:92-112.  Only buffer() is public upstream; the
    other fields are what its Debug output shows, plus (chunk, j, try_phase)."""
    msg: bytes          # all 14 sliced bytes
    msglen: int         # 7 (MsgLen::Short) | 14 (MsgLen::Long)
    signal_level: float
    score: int
    j: int = 0
    try_phase: int = 0
    chunk: int = 0

    def buffer(self) -> bytes:  # src/demod_2400.rs:106-111
        return self.msg[: self.msglen]


_MSG_STRUCT = struct.Struct("<14sBBiIQd")   # adsb_msg (include/adsb_hip.h): msg, len, try_phase, score, j, chunk, signal_level
assert _MSG_STRUCT.size == C.sizeof(AdsbMsg)


def _as_iq(iq) -> np.ndarray:
    """Accept (N,2) int16 [re, im] rows, flat interleaved int16, or complex arrays of ints."""
    if type(iq) is np.ndarray and iq.dtype == np.int16 and iq.ndim == 2 and iq.shape[1] == 2 and iq.flags.c_contiguous:
        return iq
    a = np.asarray(iq)
    if np.iscomplexobj(a):
        a = np.stack([a.real, a.imag], axis=-1)
    a = np.ascontiguousarray(a, dtype=np.int16)
    if a.ndim == 1:
        if a.size % 2:
            raise ValueError("interleaved IQ needs an even number of int16")
        a = a.reshape(-1, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("IQ must be (N, 2) int16 rows of [re, im]")
    return a


def _as_cu8(iq) -> np.ndarray:
    """CU8 input: (N, 2) uint8 rows of [re, im] or flat interleaved bytes (rtl_sdr's I, Q order)."""
    a = np.asarray(iq)
    if a.dtype != np.uint8:
        raise TypeError("CU8 IQ must be a uint8 array")
    a = np.ascontiguousarray(a)
    if a.ndim == 1:
        if a.size % 2:
            raise ValueError("interleaved CU8 IQ needs an even number of bytes")
        a = a.reshape(-1, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("CU8 IQ must be (N, 2) uint8 rows of [re, im]")
    return a


def _as_cf32(iq) -> np.ndarray:
    """CF32 input: a 1-D complex64 array, (N, 2) float32 rows of [re, im] or flat interleaved float32."""
    a = np.asarray(iq)
    if a.dtype == np.complex64:
        if a.ndim != 1:
            raise ValueError("complex64 IQ must be 1-D")
        return np.ascontiguousarray(a).view(np.float32).reshape(-1, 2)
    if a.dtype != np.float32:
        raise TypeError("CF32 IQ must be a float32 or complex64 array")
    a = np.ascontiguousarray(a)
    if a.ndim == 1:
        if a.size % 2:
            raise ValueError("interleaved CF32 IQ needs an even number of float32")
        a = a.reshape(-1, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("CF32 IQ must be (N, 2) float32 rows of [re, im]")
    return a


def _as_real16(samples) -> np.ndarray:
    """REAL16 input: a 1-D int16 array, one real sample each."""
    a = np.asarray(samples)
    if a.dtype != np.int16:
        raise TypeError("real samples must be an int16 array")
    if a.ndim != 1:
        raise ValueError("real samples must be 1-D: one int16 per sample")
    return np.ascontiguousarray(a)


def _as_format(iq, format: int) -> np.ndarray:
    """The host array of a decimator's or resampler's input in `format`; shape[0] is its sample count."""
    if format == _lib.ADSB_DECIM_CS16:
        return _as_iq(iq)
    if format == _lib.ADSB_DECIM_8BIT:
        return _as_cu8(iq)
    if format == _lib.ADSB_DECIM_CF32:
        return _as_cf32(iq)
    if format == _lib.ADSB_DECIM_REAL16:
        return _as_real16(iq)
    raise ValueError(f"no such sample format: {format}")


def _set_scale(handle, call, what: str, scale) -> None:
    handle._check(call(handle._h, C.c_float(float(scale))), what)


# adsb_trial as a numpy record (32 bytes)
TRIAL_DTYPE = np.dtype([("power", "<u8"), ("chunk", "<u4"), ("j_tp", "<u4"), ("msg", "u1", (14,)), ("pad", "<u2")])


# adsb_signal_stats as a numpy record (272 bytes)
SIGNAL_STATS_DTYPE = np.dtype([("chunk", "<u8"), ("sum_power", "<u8"), ("n_samples", "<u4"), ("peak", "<u4"),
                               ("n_strong", "<u4"), ("n_clipped", "<u4"), ("hist", "<u4", (60,))])
assert SIGNAL_STATS_DTYPE.itemsize == C.sizeof(_lib.AdsbSignalStats) == 272


def signal_summary(records: np.ndarray) -> dict:
    """adsb_signal_summary over any number of signal records (host only): buffers, samples, mean power, peak and
    median (the noise floor) in dBFS, and the clipped and strong fractions."""
    rec = np.ascontiguousarray(records, dtype=SIGNAL_STATS_DTYPE)
    out = _lib.AdsbSignalSummary()
    st = _lib.lib().adsb_signal_summary(rec.ctypes.data if rec.size else None, rec.size, C.byref(out))
    if st != _lib.ADSB_OK:
        raise AdsbError(st, "adsb_signal_summary")
    return {name: getattr(out, name) for name, _ in _lib.AdsbSignalSummary._fields_}


# adsb_input_stats as a numpy record (208 bytes)
INPUT_STATS_DTYPE = np.dtype([("n_samples", "<u8"), ("sum_re", "<i8"), ("sum_im", "<i8"), ("sum_re2", "<u8"), ("sum_im2", "<u8"),
                              ("sum_re_im", "<i8"), ("n_clipped", "<u8"), ("n_nan", "<u8"), ("hist", "<u8", (_lib.ADSB_INPUT_BINS,)),
                              ("peak", "<u4"), ("reserved", "<u4")])
assert INPUT_STATS_DTYPE.itemsize == C.sizeof(_lib.AdsbInputStats) == 208


def input_summary(records: np.ndarray) -> dict:
    """adsb_input_summary over any number of input records (host only): mean power and peak in dBFS, the DC offset in
    LSB, the clipped and NaN fractions, the I/Q gain balance in dB and the bits in use."""
    rec = np.ascontiguousarray(records, dtype=INPUT_STATS_DTYPE).reshape(-1)
    out = _lib.AdsbInputSummary()
    ptr = rec.ctypes.data_as(C.POINTER(_lib.AdsbInputStats)) if rec.size else None
    st = _lib.lib().adsb_input_summary(ptr, rec.size, C.byref(out))
    if st != _lib.ADSB_OK:
        raise AdsbError(st, "adsb_input_summary")
    return {name: getattr(out, name) for name, _ in _lib.AdsbInputSummary._fields_ if name != "reserved"}


def _set_input_stats(handle, kind: str, enabled: bool) -> None:
    call = getattr(handle._L, f"adsb_instat_set_{kind}")
    handle._check(call(handle._h, 1 if enabled else 0), f"adsb_instat_set_{kind}")


def _input_stats(handle, kind: str, first: Optional[int] = None, n: Optional[int] = None) -> np.ndarray:
    out = np.zeros(1 if n is None else int(n), dtype=INPUT_STATS_DTYPE)
    ptr = out.ctypes.data_as(C.POINTER(_lib.AdsbInputStats))
    call = getattr(handle._L, f"adsb_instat_fetch_{kind}")
    st = call(handle._h, ptr) if first is None else call(handle._h, int(first), int(n), ptr)
    handle._check(st, f"adsb_instat_fetch_{kind}")
    return out


def replay_records(records: np.ndarray, filter_table: Optional[np.ndarray] = None, cap: Optional[int] = None,
                   mode: int = 0) -> List["ModeSMessage"]:
    """adsb_replay_records: the ordered host replay (scoring + best-of-5 + ICAO filter) over raw
    trial records; `filter_table` (4096 u32, table A of the filter) is read and updated.  `mode`: the
    error-correction mode (adsb_replay_records_fix; _lib.ADSB_FIX_NONE is adsb_replay_records itself)."""
    L = _lib.lib()
    rec = np.ascontiguousarray(records, dtype=TRIAL_DTYPE).copy()
    table = filter_table if filter_table is not None else np.zeros(4096, dtype=np.uint32)
    assert table.dtype == np.uint32 and table.shape == (4096,) and table.flags.c_contiguous
    cap = cap or max(4096, rec.shape[0])
    out = (AdsbMsg * cap)()
    n = C.c_size_t()
    if mode == _lib.ADSB_FIX_NONE:
        st = L.adsb_replay_records(table.ctypes.data, rec.ctypes.data, rec.shape[0], out, cap, C.byref(n))
    else:
        st = L.adsb_replay_records_fix(table.ctypes.data, rec.ctypes.data, rec.shape[0], int(mode), out, cap, C.byref(n))
    if st != _lib.ADSB_OK:
        raise AdsbError(st, f"adsb_replay_records: {L.adsb_strerror(st).decode()}")
    return [ModeSMessage(bytes(m.msg), int(m.len), float(m.signal_level), int(m.score), int(m.j),
                         int(m.try_phase), int(m.chunk)) for m in out[: n.value]]


def _as_map(receivers, n_samples: Optional[int] = None) -> np.ndarray:
    """The receiver of every buffer of a call as the library takes it: uint32, C-contiguous (converted otherwise), one
    entry per 131072-sample buffer."""
    m = np.ascontiguousarray(receivers, dtype=np.uint32)
    if m.ndim != 1:
        raise ValueError("the receiver map is a flat array, one entry per buffer")
    if n_samples is not None and m.shape[0] < -(-n_samples // MODES_MAG_BUF_SAMPLES):
        raise ValueError(f"the receiver map names {m.shape[0]} buffers, the call has {-(-n_samples // MODES_MAG_BUF_SAMPLES)}")
    return m


def rx_set_home(key: int, set_lg: int) -> int:
    """adsb_rx_set_home (host only): the slot the probes of key = receiver << 24 | value start at in a keyed set of
    2^set_lg slots."""
    return int(_lib.lib().adsb_rx_set_home(int(key), int(set_lg)))


def replay_records_rx(records: np.ndarray, receivers, filter_tables: np.ndarray, mode: int = 0, threads: int = 1,
                      cap: Optional[int] = None) -> List["ModeSMessage"]:
    """adsb_replay_records_rx: the ordered host replay with one filter per receiver.  `receivers[b]` is the receiver of
    buffer b (the records' `chunk`); `filter_tables` ((n_receivers, 4096) u32, table A of every filter) is read and
    updated.  threads > 1: the receivers dealt to that many threads -- the same result."""
    L = _lib.lib()
    rec = np.ascontiguousarray(records, dtype=TRIAL_DTYPE).copy()
    m = _as_map(receivers)
    assert filter_tables.dtype == np.uint32 and filter_tables.ndim == 2 and filter_tables.shape[1] == 4096 \
        and filter_tables.flags.c_contiguous
    cap = cap or max(4096, rec.shape[0])
    out = (AdsbMsg * cap)()
    n = C.c_size_t()
    st = L.adsb_replay_records_rx(filter_tables.ctypes.data, filter_tables.shape[0], m.ctypes.data if m.size else None,
                                  m.shape[0], rec.ctypes.data if rec.size else None, rec.shape[0], int(mode), int(threads),
                                  out, cap, C.byref(n))
    if st != _lib.ADSB_OK:
        raise AdsbError(st, f"adsb_replay_records_rx: {L.adsb_strerror(st).decode()}")
    return [ModeSMessage(bytes(x.msg), int(x.len), float(x.signal_level), int(x.score), int(x.j),
                         int(x.try_phase), int(x.chunk)) for x in out[: n.value]]


class Context:
    """One adsb_ctx: device buffers, stream and the ICAO filter of one stream of IQ."""

    def __init__(self, device: int = 0, max_chunks: int = 1):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        st = self._L.adsb_create(C.byref(self._h), int(device), int(max_chunks))
        if st != _lib.ADSB_OK:
            self._h = C.c_void_p()
            raise AdsbError(st, "adsb_create", self._L.adsb_strerror(st).decode())
        self.device = device
        self.max_chunks = max_chunks

    # -- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._L.adsb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st: int, what: str) -> None:
        if st != _lib.ADSB_OK:
            detail = self._L.adsb_last_error(self._h).decode() if st == _lib.ADSB_ERR_HIP else ""
            raise AdsbError(st, f"{what}: {self._L.adsb_strerror(st).decode()}", detail)

    # -- reference API
    def icao_flush(self) -> None:
        self._check(self._L.adsb_icao_flush(self._h), "adsb_icao_flush")

    def to_mag(self, iq) -> MagnitudeBuffer:
        a = _as_iq(iq)
        # (the library writes all 131398 entries, lead-in and tail zeros included: no need to zero them first)
        out = MagnitudeBuffer(data=np.empty(MAG_DATA_LEN, dtype=np.uint16))
        n = C.c_size_t()
        st = self._L.adsb_to_mag(self._h, a.__array_interface__["data"][0], a.shape[0],
                                 out.data.__array_interface__["data"][0], C.byref(n))
        if st == _lib.ADSB_ERR_TOO_LONG:
            raise IndexError("to_mag: more than 131072 samples (the reference panics here)")
        self._check(st, "adsb_to_mag")
        out.length = n.value
        return out

    # -- 8-bit IQ (CU8, an RTL-SDR's samples): each call returns what its CS16 twin returns on the samples widened
    #    through the context's table (include/adsb_hip.h, "8-bit IQ")
    def set_u8_table(self, table=None) -> None:
        """The widening table from now on: 256 int16, or None for T_soapy (a new context's)."""
        if table is None:
            self._check(self._L.adsb_set_u8_table(self._h, None), "adsb_set_u8_table")
            return
        t = np.ascontiguousarray(table, dtype=np.int16)
        if t.shape != (256,):
            raise ValueError("the CU8 table holds 256 int16")
        self._check(self._L.adsb_set_u8_table(self._h, t.ctypes.data), "adsb_set_u8_table")

    def u8_table(self) -> np.ndarray:
        """The table the context widens with (adsb_selftest_u8_table)."""
        out = np.empty(256, dtype=np.int16)
        self._check(self._L.adsb_selftest_u8_table(self._h, out.ctypes.data), "adsb_selftest_u8_table")
        return out

    def to_mag_u8(self, iq) -> MagnitudeBuffer:
        a = _as_cu8(iq)
        out = MagnitudeBuffer(data=np.empty(MAG_DATA_LEN, dtype=np.uint16))
        n = C.c_size_t()
        st = self._L.adsb_to_mag_u8(self._h, a.ctypes.data, a.shape[0], out.data.ctypes.data, C.byref(n))
        if st == _lib.ADSB_ERR_TOO_LONG:
            raise IndexError("to_mag_u8: more than 131072 samples (the reference panics here)")
        self._check(st, "adsb_to_mag_u8")
        out.length = n.value
        return out

    def demod_iq_u8(self, iq, cap: Optional[int] = None) -> List[ModeSMessage]:
        a = _as_cu8(iq)
        cap = cap or max(4096, a.shape[0] // 256)
        ptr = a.ctypes.data
        return self._collect(
            lambda out, c, n: self._L.adsb_demod_iq_u8(self._h, ptr, a.shape[0], out, c, n), "adsb_demod_iq_u8", cap)

    def demod_iq_device_u8(self, device_ptr: int, n_samples: int, cap: Optional[int] = None) -> List[ModeSMessage]:
        cap = cap or max(4096, n_samples // 256)
        return self._collect(
            lambda out, c, n: self._L.adsb_demod_iq_device_u8(self._h, C.c_void_p(device_ptr), n_samples, out, c, n),
            "adsb_demod_iq_device_u8", cap)

    def submit_iq_device_u8(self, device_ptr: int, n_samples: int) -> None:
        self._check(self._L.adsb_submit_iq_device_u8(self._h, C.c_void_p(device_ptr), n_samples),
                    "adsb_submit_iq_device_u8")

    def ring_create_u8(self, samples_per_slot: int) -> None:
        self._check(self._L.adsb_ring_create_u8(self._h, samples_per_slot), "adsb_ring_create_u8")

    def ring_acquire_u8(self) -> np.ndarray:
        """The pinned (capacity, 2) uint8 [re, im] buffer of the next submission of a CU8 ring."""
        ptr, cap = C.c_void_p(), C.c_size_t()
        self._check(self._L.adsb_ring_acquire_u8(self._h, C.byref(ptr), C.byref(cap)), "adsb_ring_acquire_u8")
        buf = (C.c_uint8 * (2 * cap.value)).from_address(ptr.value)
        return np.ctypeslib.as_array(buf).reshape(-1, 2)

    def _collect(self, call, what: str, cap: int) -> List[ModeSMessage]:
        # (the output array is kept between calls: allocating and zeroing 4096 entries costs more than
        # a one-buffer pass takes)
        if getattr(self, "_out_cap", 0) != cap:
            self._out_buf, self._out_cap = (AdsbMsg * cap)(), cap
            self._out_view = memoryview(self._out_buf).cast("B")
        buf, view = self._out_buf, self._out_view
        n = C.c_size_t()
        st = call(buf, cap, C.byref(n))
        if st == _lib.ADSB_ERR_CAPACITY:
            # the pass is consumed (the filter has advanced): never repeat the call, fetch its list
            cap = n.value
            buf = (AdsbMsg * cap)()
            view = memoryview(buf).cast("B")
            st = self._L.adsb_fetch_messages(self._h, buf, cap, C.byref(n))
        self._check(st, what)
        # (adsb_msg unpacked in one go: field by field through ctypes a list of five messages cost 11 us, more
        # than a quarter of the call that produced it)
        return [ModeSMessage(m, ln, sig, score, j, tp, chunk)
                for (m, ln, tp, score, j, chunk, sig) in _MSG_STRUCT.iter_unpack(view[: _MSG_STRUCT.size * n.value])]

    def demodulate2400(self, mag: MagnitudeBuffer, cap: int = 4096) -> List[ModeSMessage]:
        data = np.ascontiguousarray(mag.data, dtype=np.uint16)
        if data.shape != (MAG_DATA_LEN,):
            raise ValueError("MagnitudeBuffer.data must hold 131398 u16")
        if mag.length > MODES_MAG_BUF_SAMPLES:
            raise IndexError("MagnitudeBuffer.length > 131072")
        return self._collect(
            lambda out, c, n: self._L.adsb_demodulate2400(self._h, data.__array_interface__["data"][0], mag.length, out, c, n),
            "adsb_demodulate2400", cap)

    # -- stream forms (to_mag + demodulate2400 per 131072-sample buffer)
    def demod_iq(self, iq, cap: Optional[int] = None) -> List[ModeSMessage]:
        a = _as_iq(iq)
        cap = cap or max(4096, a.shape[0] // 256)
        ptr = a.__array_interface__["data"][0]   # (a.ctypes.data builds an object per call: 1.8 us against 1.1)
        return self._collect(
            lambda out, c, n: self._L.adsb_demod_iq(self._h, ptr, a.shape[0], out, c, n),
            "adsb_demod_iq", cap)

    def demod_iq_device(self, device_ptr: int, n_samples: int, cap: Optional[int] = None
                        ) -> List[ModeSMessage]:
        cap = cap or max(4096, n_samples // 256)
        return self._collect(
            lambda out, c, n: self._L.adsb_demod_iq_device(self._h, C.c_void_p(device_ptr), n_samples, out, c, n),
            "adsb_demod_iq_device", cap)

    def demod_iq_device_raw(self, device_ptr: int, n_samples: int, out_buf, cap: int) -> int:
        """No Python-side unpacking: for the bench loop.  Returns the message count."""
        n = C.c_size_t()
        st = self._L.adsb_demod_iq_device(self._h, C.c_void_p(device_ptr), n_samples, out_buf, cap, C.byref(n))
        self._check(st, "adsb_demod_iq_device")
        return n.value

    # -- pipelined form: keep up to four passes in flight (ADSB_MAX_IN_FLIGHT), results in submission order
    def submit_iq_device(self, device_ptr: int, n_samples: int) -> None:
        self._check(self._L.adsb_submit_iq_device(self._h, C.c_void_p(device_ptr), n_samples),
                    "adsb_submit_iq_device")

    def decimator(self, factor: int, taps=None, shift: Optional[int] = None, shift_hz: Optional[int] = None) -> "Decimator":
        """An integer FIR decimator in front of this context's passes, for IQ sampled at factor x 2.4 MS/s
        (include/adsb_hip.h, "Decimation").  taps=None: default_taps(factor).  shift_hz: for an offset-tuned radio, how
        far the spectrum is to be moved ("Frequency shift"): the mixer of mixer_for_shift(1, factor, shift_hz) is set."""
        d = Decimator(self, factor, taps, shift)
        if shift_hz is not None:
            d.set_mixer(mixer_table(*mixer_for_shift(1, factor, shift_hz)))
        return d

    def resampler(self, up: int, down: int, taps=None, shift: Optional[int] = None, shift_hz: Optional[int] = None) -> "Resampler":
        """An exact-integer up / down resampler in front of this context's passes, for IQ sampled at 2.4 MS/s x down / up
        (include/adsb_hip.h, "Resampling").  taps=None: default_resampler_taps(up, down).  shift_hz: as for decimator(),
        with mixer_for_shift(up, down, shift_hz)."""
        r = Resampler(self, up, down, taps, shift)
        if shift_hz is not None:
            r.set_mixer(mixer_table(*mixer_for_shift(up, down, shift_hz)))
        return r

    def resampler_bank(self, n_streams: int, up: int, down: int, taps=None, shift: Optional[int] = None,
                       shift_hz: Optional[int] = None) -> "ResamplerBank":
        """n_streams independent resampler streams of one ratio and one filter that one call advances in one launch
        (include/adsb_hip.h, "Resampler banks"): each stream is a resampler() of the same arguments.  taps, shift and
        shift_hz as for resampler()."""
        b = ResamplerBank(self, n_streams, up, down, taps, shift)
        if shift_hz is not None:
            b.set_mixer(mixer_table(*mixer_for_shift(up, down, shift_hz)))
        return b

    def converter(self, scale: Optional[float] = None) -> "Resampler":
        """The 1/1 resampler with the single tap 1 and shift 0 -- the identity on CS16 -- for CF32 (or REAL16, 8-bit)
        input that is already at 2.4 MS/s (include/adsb_hip.h, "Sample formats"): converter().demod_iq(x,
        format=ADSB_DECIM_CF32) is demod_iq on q(x).  scale: g of q, 32768 by default."""
        r = Resampler(self, 1, 1, np.array([1], dtype=np.int16), 0)
        if scale is not None:
            r.set_scale(scale)
        return r

    def collect_raw(self, out_buf, cap: int) -> int:
        n = C.c_size_t()
        self._check(self._L.adsb_collect(self._h, out_buf, cap, C.byref(n)), "adsb_collect")
        return n.value

    def collect(self, cap: int = 1 << 16) -> List[ModeSMessage]:
        return self._collect(lambda out, c, n: self._L.adsb_collect(self._h, out, c, n), "adsb_collect", cap)

    def selftest_stage_lists(self, device_ptr: int, n_samples: int):
        """adsb_selftest_stage_lists: (candidate positions as buffer << 32 | j, address/parity trials as
        buffer << 45 | j << 28 | try_phase << 24 | residual), both ascending u64 arrays."""
        cc, ac = max(4096, n_samples // 16), max(4096, n_samples // 8)
        while True:
            cand, ap = np.zeros(cc, dtype=np.uint64), np.zeros(ac, dtype=np.uint64)
            nc, na = C.c_size_t(), C.c_size_t()
            st = self._L.adsb_selftest_stage_lists(self._h, C.c_void_p(device_ptr), n_samples, cand.ctypes.data, cc,
                                                   C.byref(nc), ap.ctypes.data, ac, C.byref(na))
            if st == _lib.ADSB_ERR_CAPACITY:
                cc, ac = max(cc, nc.value), max(ac, na.value)
                continue
            self._check(st, "adsb_selftest_stage_lists")
            return cand[: nc.value].copy(), ap[: na.value].copy()

    def selftest_fix_lookup(self, residuals, mode: int) -> np.ndarray:
        """adsb_selftest_fix_lookup: per CRC residual the repair the scoring kernels find under `mode`, as a | b << 8
        (0xFF | b << 8: the single bit b; 0xFFFF: none)."""
        r = np.ascontiguousarray(residuals, dtype=np.uint32)
        out = np.zeros(r.shape[0], dtype=np.uint32)
        self._check(self._L.adsb_selftest_fix_lookup(self._h, r.ctypes.data, r.shape[0], int(mode), out.ctypes.data),
                    "adsb_selftest_fix_lookup")
        return out

    def selftest_gate_stages(self, device_ptr: int, n_samples: int):
        """adsb_selftest_gate_stages: (positions where check_preamble returns Some, those that also pass
        the 3.5 dB test), both as buffer << 32 | j, ascending u64 arrays."""
        pc, sc = max(4096, n_samples // 8), max(4096, n_samples // 16)
        while True:
            pre, snr = np.zeros(pc, dtype=np.uint64), np.zeros(sc, dtype=np.uint64)
            npre, nsnr = C.c_size_t(), C.c_size_t()
            st = self._L.adsb_selftest_gate_stages(self._h, C.c_void_p(device_ptr), n_samples, pre.ctypes.data, pc,
                                                   C.byref(npre), snr.ctypes.data, sc, C.byref(nsnr))
            if st == _lib.ADSB_ERR_CAPACITY:
                pc, sc = max(pc, npre.value), max(sc, nsnr.value)
                continue
            self._check(st, "adsb_selftest_gate_stages")
            return pre[: npre.value].copy(), snr[: nsnr.value].copy()

    # -- sharded capture: two phases around a host-side exchange of learned addresses
    def shard_scan(self, device_ptr: int, n_samples: int) -> np.ndarray:
        """Phase 1 on this shard: the addresses its clean DF11 / DF17 frames will add (sorted u32)."""
        cap = 1 << 16
        while True:
            out = np.zeros(cap, dtype=np.uint32)
            n = C.c_size_t()
            st = self._L.adsb_shard_scan(self._h, C.c_void_p(device_ptr), n_samples, out.ctypes.data, cap,
                                         C.byref(n))
            if st == _lib.ADSB_ERR_CAPACITY:  # the shard stays parked: finish it, then retry bigger
                self._L.adsb_shard_finish(self._h, None, 0, None, 0, None)
                cap = n.value
                continue
            self._check(st, "adsb_shard_scan")
            return out[: n.value].copy()

    def shard_finish(self, extra_addrs, cap: Optional[int] = None) -> np.ndarray:
        """Phase 2: add the other shards' addresses, match, return the raw trial records
        (structured array with the layout of adsb_trial; `chunk` is local to the shard)."""
        extra = np.ascontiguousarray(extra_addrs, dtype=np.uint32)
        cap = cap or (1 << 20)
        rec = np.zeros(cap, dtype=TRIAL_DTYPE)
        n = C.c_size_t()
        st = self._L.adsb_shard_finish(self._h, extra.ctypes.data if extra.size else None, extra.size,
                                       rec.ctypes.data, cap, C.byref(n))
        if st == _lib.ADSB_ERR_CAPACITY:
            raise AdsbError(st, f"adsb_shard_finish: {n.value} records exceed cap {cap}")
        self._check(st, "adsb_shard_finish")
        return rec[: n.value].copy()

    # -- a buffer the caller keeps (main.rs:154-167 reads the SDR into one Vec for ever): pinned and mapped once,
    #    demod_iq on samples inside it reads them in place
    def host_register(self, a: np.ndarray) -> None:
        self._check(self._L.adsb_host_register(self._h, a.ctypes.data, a.nbytes), "adsb_host_register")

    def host_unregister(self, a: np.ndarray) -> None:
        self._check(self._L.adsb_host_unregister(self._h, a.ctypes.data), "adsb_host_unregister")

    # -- streaming ring: pinned host buffers, H2D overlapped with the other slot's pass
    def ring_create(self, samples_per_slot: int) -> None:
        self._check(self._L.adsb_ring_create(self._h, samples_per_slot), "adsb_ring_create")

    def ring_acquire(self) -> np.ndarray:
        """The pinned (capacity, 2) int16 [re, im] buffer of the next submission."""
        ptr, cap = C.c_void_p(), C.c_size_t()
        self._check(self._L.adsb_ring_acquire(self._h, C.byref(ptr), C.byref(cap)), "adsb_ring_acquire")
        buf = (C.c_int16 * (2 * cap.value)).from_address(ptr.value)
        return np.ctypeslib.as_array(buf).reshape(-1, 2)

    def ring_acquire_raw(self) -> int:
        """adsb_ring_acquire without wrapping the buffer in an array (a host loop whose slots are already
        filled): the buffer's address."""
        if not hasattr(self, "_ring_ptr"):
            self._ring_ptr, self._ring_cap = C.c_void_p(), C.c_size_t()
        self._check(self._L.adsb_ring_acquire(self._h, C.byref(self._ring_ptr), C.byref(self._ring_cap)), "adsb_ring_acquire")
        return self._ring_ptr.value

    def ring_submit(self, n_samples: int) -> None:
        self._check(self._L.adsb_ring_submit(self._h, n_samples), "adsb_ring_submit")

    # -- many receivers, one pass: one ICAO filter per receiver, `receivers[b]` names the receiver of buffer b of a call
    #    (include/adsb_hip.h, "Many receivers, one pass")
    def set_receivers(self, n: int) -> None:
        """adsb_set_receivers: n filters (0: off); every receiver restarts from an empty filter."""
        self._check(self._L.adsb_set_receivers(self._h, int(n)), "adsb_set_receivers")

    def receivers(self) -> int:
        return int(self._L.adsb_get_receivers(self._h))

    def icao_flush_receiver(self, r: int) -> None:
        """icao_flush() for receiver r alone, for the passes submitted after it."""
        self._check(self._L.adsb_icao_flush_receiver(self._h, int(r)), "adsb_icao_flush_receiver")

    def receiver_filter_table(self, r: int) -> np.ndarray:
        """Table A (4096 u32) of receiver r's filter."""
        out = np.zeros(4096, dtype=np.uint32)
        self._check(self._L.adsb_receiver_filter_table(self._h, int(r), out.ctypes.data), "adsb_receiver_filter_table")
        return out

    def demod_iq_rx(self, iq, receivers, cap: Optional[int] = None) -> List[ModeSMessage]:
        a = _as_iq(iq)
        m = _as_map(receivers, a.shape[0])
        cap = cap or max(4096, a.shape[0] // 256)
        return self._collect(
            lambda out, c, n: self._L.adsb_demod_iq_rx(self._h, a.ctypes.data, a.shape[0], m.ctypes.data, out, c, n),
            "adsb_demod_iq_rx", cap)

    def demod_iq_rx_u8(self, iq, receivers, cap: Optional[int] = None) -> List[ModeSMessage]:
        a = _as_cu8(iq)
        m = _as_map(receivers, a.shape[0])
        cap = cap or max(4096, a.shape[0] // 256)
        return self._collect(
            lambda out, c, n: self._L.adsb_demod_iq_rx_u8(self._h, a.ctypes.data, a.shape[0], m.ctypes.data, out, c, n),
            "adsb_demod_iq_rx_u8", cap)

    def demod_iq_device_rx(self, device_ptr: int, n_samples: int, receivers, cap: Optional[int] = None) -> List[ModeSMessage]:
        m = _as_map(receivers, n_samples)
        cap = cap or max(4096, n_samples // 256)
        return self._collect(
            lambda out, c, n: self._L.adsb_demod_iq_device_rx(self._h, C.c_void_p(device_ptr), n_samples, m.ctypes.data, out, c, n),
            "adsb_demod_iq_device_rx", cap)

    def demod_iq_device_rx_u8(self, device_ptr: int, n_samples: int, receivers, cap: Optional[int] = None) -> List[ModeSMessage]:
        m = _as_map(receivers, n_samples)
        cap = cap or max(4096, n_samples // 256)
        return self._collect(
            lambda out, c, n: self._L.adsb_demod_iq_device_rx_u8(self._h, C.c_void_p(device_ptr), n_samples, m.ctypes.data, out, c, n),
            "adsb_demod_iq_device_rx_u8", cap)

    def submit_iq_device_rx(self, device_ptr: int, n_samples: int, receivers) -> None:
        m = _as_map(receivers, n_samples)   # (copied by the call: it need not outlive it)
        self._check(self._L.adsb_submit_iq_device_rx(self._h, C.c_void_p(device_ptr), n_samples, m.ctypes.data),
                    "adsb_submit_iq_device_rx")

    def submit_iq_device_rx_u8(self, device_ptr: int, n_samples: int, receivers) -> None:
        m = _as_map(receivers, n_samples)
        self._check(self._L.adsb_submit_iq_device_rx_u8(self._h, C.c_void_p(device_ptr), n_samples, m.ctypes.data),
                    "adsb_submit_iq_device_rx_u8")

    def ring_submit_rx(self, n_samples: int, receivers) -> None:
        m = _as_map(receivers, n_samples)
        self._check(self._L.adsb_ring_submit_rx(self._h, n_samples, m.ctypes.data), "adsb_ring_submit_rx")

    def set_receiver_carry(self, enabled: bool) -> None:
        """adsb_set_receiver_carry: carry-over with receivers on -- every buffer's lead-in is the end of its own receiver's
        previous buffer (include/adsb_hip.h, "Receiver seams")."""
        self._check(self._L.adsb_set_receiver_carry(self._h, 1 if enabled else 0), "adsb_set_receiver_carry")

    def get_receiver_carry(self) -> bool:
        return int(self._L.adsb_get_receiver_carry(self._h)) == 1

    def receiver_carry_reset(self, receiver: int = RX_ALL) -> None:
        """adsb_receiver_carry_reset: nothing precedes the next buffer of `receiver` (default: of every receiver)."""
        self._check(self._L.adsb_receiver_carry_reset(self._h, receiver), "adsb_receiver_carry_reset")

    def selftest_rx_seam_tune(self, list_cap: int = 0) -> None:
        self._check(self._L.adsb_selftest_rx_seam_tune(self._h, list_cap), "adsb_selftest_rx_seam_tune")

    def selftest_rx_seam_counters(self) -> dict:
        """adsb_selftest_rx_seam_counters: passes with a seam step / seam records handed to the replay / records of the
        pass itself dropped for j < 326 / seam steps redone after an overflow."""
        out = (C.c_uint64 * 4)()
        self._check(self._L.adsb_selftest_rx_seam_counters(self._h, out), "adsb_selftest_rx_seam_counters")
        return {"passes": int(out[0]), "records": int(out[1]), "dropped": int(out[2]), "redone": int(out[3])}

    def set_receiver_carry_scoring(self, enabled: bool) -> None:
        """adsb_set_receiver_carry_scoring: receiver seams AND per-receiver scoring on the device, entered and left
        together (include/adsb_hip.h, "Receiver seams, scored on the device")."""
        self._check(self._L.adsb_set_receiver_carry_scoring(self._h, 1 if enabled else 0), "adsb_set_receiver_carry_scoring")

    def get_receiver_carry_scoring(self) -> bool:
        return int(self._L.adsb_get_receiver_carry_scoring(self._h)) == 1

    def selftest_rx_seam_score_counters(self) -> dict:
        """adsb_selftest_rx_seam_score_counters: passes with a device-side seam merge / seam records merged on the device /
        own hits dropped there for j < 326 / merged passes that declared themselves unscored."""
        out = (C.c_uint64 * 4)()
        self._check(self._L.adsb_selftest_rx_seam_score_counters(self._h, out), "adsb_selftest_rx_seam_score_counters")
        return {"merged_passes": int(out[0]), "seam_records": int(out[1]), "dropped": int(out[2]), "unscored": int(out[3])}

    def selftest_reservations(self) -> int:
        """adsb_selftest_reservations: what the context's owner holds now (device blocks, pinned blocks and events)."""
        return int(self._L.adsb_selftest_reservations(self._h))

    def set_receiver_scoring(self, enabled: bool) -> None:
        """adsb_set_receiver_scoring: dense passes of a receivers context are scored on the device, a filter per receiver."""
        self._check(self._L.adsb_set_receiver_scoring(self._h, 1 if enabled else 0), "adsb_set_receiver_scoring")

    def get_receiver_scoring(self) -> bool:
        return int(self._L.adsb_get_receiver_scoring(self._h)) == 1

    def selftest_rx_score_counters(self) -> dict:
        """adsb_selftest_rx_score_counters: device results taken / scored passes the host replayed all the same / rebuilds
        of the keyed set / passes in which an insertion ran out of probes."""
        out = (C.c_uint64 * 4)()
        self._check(self._L.adsb_selftest_rx_score_counters(self._h, out), "adsb_selftest_rx_score_counters")
        return {"taken": int(out[0]), "refused": int(out[1]), "rebuilds": int(out[2]), "no_room": int(out[3])}

    def selftest_rx_score_tune(self, set_lg: int = 0, probe_max: int = 0) -> None:
        self._check(self._L.adsb_selftest_rx_score_tune(self._h, int(set_lg), int(probe_max)), "adsb_selftest_rx_score_tune")

    def selftest_rx_set_lookup(self, keys, queries):
        """adsb_selftest_rx_set_lookup: (found[len(queries)] as a bool array, insertions that ran out of probes)."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        q = np.ascontiguousarray(queries, dtype=np.uint64)
        out = np.zeros(q.shape[0] + 1, dtype=np.uint32)
        self._check(self._L.adsb_selftest_rx_set_lookup(self._h, k.ctypes.data, k.shape[0], q.ctypes.data, q.shape[0], out.ctypes.data),
                    "adsb_selftest_rx_set_lookup")
        return out[:-1].astype(bool), int(out[-1])

    def selftest_rx_tune(self, parallel_min: int = 0) -> None:
        self._check(self._L.adsb_selftest_rx_tune(self._h, int(parallel_min)), "adsb_selftest_rx_tune")

    def selftest_rx_counters(self) -> dict:
        """adsb_selftest_rx_counters: passes replayed per receiver, those of them replayed by several threads, and how
        often the device's superset was put back from the union of the receivers' filters."""
        out = (C.c_uint64 * 4)()
        self._check(self._L.adsb_selftest_rx_counters(self._h, out), "adsb_selftest_rx_counters")
        return {"rx_passes": int(out[0]), "pooled_passes": int(out[1]), "union_reseeds": int(out[2])}

    def pending(self) -> int:
        return int(self._L.adsb_pending(self._h))
    def pending(self) -> int:
        return int(self._L.adsb_pending(self._h))

    def max_in_flight(self) -> int:
        """4, or 8 for a context created for at most 16 buffers per pass (adsb_max_in_flight)."""
        return int(self._L.adsb_max_in_flight(self._h))

    def set_stream(self, hip_stream: int) -> None:
        self._check(self._L.adsb_set_stream(self._h, C.c_void_p(hip_stream)), "adsb_set_stream")

    def set_carry_over(self, enabled: bool) -> None:
        """Opt-in, not the reference's semantics: buffer lead-ins hold the preceding samples."""
        self._check(self._L.adsb_set_carry_over(self._h, 1 if enabled else 0), "adsb_set_carry_over")

    def set_error_correction(self, mode: int) -> None:
        """adsb_set_error_correction: _lib.ADSB_FIX_NONE (default, the reference), _lib.ADSB_FIX_1BIT (single-bit
        repair of DF17/18 from known aircraft, score _lib.ADSB_SCORE_FIXED_1BIT) or _lib.ADSB_FIX_2BIT (one or two
        flipped bits; a two-bit repair scores _lib.ADSB_SCORE_FIXED_2BIT); for the passes submitted after it."""
        self._check(self._L.adsb_set_error_correction(self._h, int(mode)), "adsb_set_error_correction")

    def set_signal_stats(self, enabled: bool) -> None:
        """adsb_set_signal_stats: opt-in; the passes submitted after it also deliver one integer record per
        131072-sample buffer (signal_stats())."""
        self._check(self._L.adsb_set_signal_stats(self._h, 1 if enabled else 0), "adsb_set_signal_stats")

    def signal_stats(self) -> np.ndarray:
        """adsb_fetch_signal_stats: the records of the pass collected last (or of the blocking call returned last),
        one per buffer in buffer order, as a structured array with the layout of adsb_signal_stats; empty when
        that pass ran with the mode off."""
        n = C.c_size_t()
        st = self._L.adsb_fetch_signal_stats(self._h, None, 0, C.byref(n))
        out = np.zeros(n.value, dtype=SIGNAL_STATS_DTYPE)
        if n.value:
            st = self._L.adsb_fetch_signal_stats(self._h, out.ctypes.data, n.value, C.byref(n))
        self._check(st, "adsb_fetch_signal_stats")
        return out

    @property
    def error_correction(self) -> int:
        return int(self._L.adsb_get_error_correction(self._h))

    def set_profiling(self, level: int) -> None:
        """0 = no HIP events, 1 = scan kernel + whole chain (default), 2 = every kernel."""
        self._check(self._L.adsb_set_profiling(self._h, int(level)), "adsb_set_profiling")

    def stats_raw(self) -> AdsbStats:
        """The adsb_stats struct itself (no dict building: for tight loops)."""
        if not hasattr(self, "_stats_buf"):
            self._stats_buf = AdsbStats()
        self._check(self._L.adsb_get_stats(self._h, C.byref(self._stats_buf)), "adsb_get_stats")
        return self._stats_buf

    def stats(self) -> dict:
        s = AdsbStats()
        self._check(self._L.adsb_get_stats(self._h, C.byref(s)), "adsb_get_stats")
        return {name: getattr(s, name) for name, _ in AdsbStats._fields_ if name != "reserved"}


def mixer_table(k: int, period: int):
    """adsb_mix_table (host only): the (period, 2) int16 table {c, s} of a shift by k / period cycles per sample, amplitude
    2^14 (include/adsb_hip.h, "Frequency shift")."""
    L = _lib.lib()
    if not (0 <= int(k) < 1 << 32 and 0 <= int(period) < 1 << 32):
        raise AdsbError(_lib.ADSB_ERR_INVALID, f"adsb_mix_table: {k}/{period}")
    table = np.zeros((max(int(period), 1), 2), dtype=np.int16)
    st = L.adsb_mix_table(int(k), int(period), table.ctypes.data_as(C.POINTER(C.c_int16)), table.shape[0])
    if st != _lib.ADSB_OK:
        raise AdsbError(st, f"adsb_mix_table: {L.adsb_strerror(st).decode()}")
    return table


def mixer_for_shift(up: int, down: int, shift_hz: int):
    """adsb_mix_for_shift (host only): (k, period) of the table that moves the spectrum of a stream at 2.4 MS/s x down / up
    (a decimator: up = 1, down = factor) by shift_hz, signed.  AdsbError (ADSB_ERR_INVALID, with the terms in .terms)
    where the period is beyond 256."""
    L = _lib.lib()
    k, period = C.c_uint32(), C.c_uint32()
    if not (0 <= int(up) < 1 << 32 and 0 <= int(down) < 1 << 32 and -(1 << 31) <= int(shift_hz) < 1 << 31):
        raise AdsbError(_lib.ADSB_ERR_INVALID, f"adsb_mix_for_shift: {up}/{down}, {shift_hz} Hz")
    st = L.adsb_mix_for_shift(int(up), int(down), int(shift_hz), C.byref(k), C.byref(period))
    if st != _lib.ADSB_OK:
        err = AdsbError(st, f"adsb_mix_for_shift: {shift_hz} Hz at {up}/{down} needs {k.value}/{period.value}")
        err.terms = (k.value, period.value)
        raise err
    return k.value, period.value


def _set_mixer(handle, call, what: str, table) -> None:
    if table is None:
        handle._check(call(handle._h, None, 0), what)
        return
    t = np.ascontiguousarray(table, dtype=np.int16)
    if t.ndim != 2 or t.shape[1] != 2:
        raise ValueError("a mixer's table is (period, 2) int16: {c, s} pairs")
    handle._check(call(handle._h, t.ctypes.data, t.shape[0]), what)


def default_taps(factor: int):
    """adsb_decim_default_taps (host only): (taps int16[8 factor + 1], shift) of a Hamming-windowed sinc with its cutoff at
    1.2 MHz."""
    L = _lib.lib()
    taps = np.empty(8 * int(factor) + 1, dtype=np.int16)
    n, shift = C.c_uint32(), C.c_uint32()
    st = L.adsb_decim_default_taps(int(factor), taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size, C.byref(n), C.byref(shift))
    if st != _lib.ADSB_OK:
        raise AdsbError(st, f"adsb_decim_default_taps: {L.adsb_strerror(st).decode()}")
    return taps[: n.value], int(shift.value)


class Decimator:
    """One adsb_decim: a stateful exact-integer FIR decimator by `factor` on the context's device.  Close it before its
    context."""

    def __init__(self, ctx: Context, factor: int, taps=None, shift: Optional[int] = None):
        self._ctx, self._L = ctx, ctx._L
        self._h = C.c_void_p()
        if taps is None:
            taps, default_shift = default_taps(factor)
            shift = default_shift if shift is None else shift
        elif shift is None:
            raise ValueError("taps of the caller's need a shift")
        t = np.ascontiguousarray(taps, dtype=np.int16)
        if t.ndim != 1:
            raise ValueError("the taps are a flat int16 array")
        self.factor, self.taps, self.shift = int(factor), t, int(shift)
        self._check(self._L.adsb_decim_create(ctx._h, int(factor), t.ctypes.data, t.size, int(shift), C.byref(self._h)),
                    "adsb_decim_create")

    def _check(self, st: int, what: str) -> None:
        self._ctx._check(st, what)

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            if self._ctx._h.value:   # (a context that is gone took the device state with it)
                self._L.adsb_decim_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self) -> None:
        self._check(self._L.adsb_decim_reset(self._h), "adsb_decim_reset")

    def set_mixer(self, table) -> None:
        """adsb_mix_set_decim: the (period, 2) int16 table {c, s} the inputs consumed from now on are mixed with (None:
        no mixer)."""
        _set_mixer(self, self._L.adsb_mix_set_decim, "adsb_mix_set_decim", table)

    @property
    def mixer_period(self) -> int:
        return int(self._L.adsb_mix_get_decim(self._h))

    def set_scale(self, scale: float) -> None:
        """adsb_fmt_set_scale_decim: g of CF32 input, q(x) = clamp(rint(x g)); finite, 0 < g <= 2^31 (32768 by default)."""
        _set_scale(self, self._L.adsb_fmt_set_scale_decim, "adsb_fmt_set_scale_decim", scale)

    @property
    def scale(self) -> float:
        return float(self._L.adsb_fmt_get_scale_decim(self._h))

    def set_input_stats(self, enabled: bool) -> None:
        """adsb_instat_set_decim: opt-in; every input sample the decimator consumes from now on is counted on the device, raw,
        in front of the filter (input_stats()).  Disabling discards what was counted."""
        _set_input_stats(self, "decim", enabled)

    @property
    def input_stats_enabled(self) -> bool:
        return int(self._L.adsb_instat_get_decim(self._h)) == 1

    def input_stats(self) -> np.ndarray:
        """adsb_instat_fetch_decim: waits for the handle's calls, then returns the record of the inputs consumed since the
        previous fetch (or the enable) as a 0-d structured array with the layout of adsb_input_stats, and zeroes it."""
        return _input_stats(self, "decim")[0]

    def out_count(self, n_in: int) -> int:
        n = C.c_size_t()
        self._check(self._L.adsb_decim_out_count(self._h, int(n_in), C.byref(n)), "adsb_decim_out_count")
        return n.value

    def run_device(self, ptr_in: int, n_in: int, ptr_out: int, out_cap: int, format: int = _lib.ADSB_DECIM_CS16) -> int:
        """Device memory to device memory, enqueued without waiting; returns the output count.  AdsbError with status
        ADSB_ERR_CAPACITY (and the required count in .required) when out_cap is too small: nothing was consumed."""
        n = C.c_size_t()
        st = self._L.adsb_decim_run_device(self._h, int(format), C.c_void_p(ptr_in), int(n_in), C.c_void_p(ptr_out), int(out_cap),
                                           C.byref(n))
        if st == _lib.ADSB_ERR_CAPACITY:
            err = AdsbError(st, f"adsb_decim_run_device: {n.value} outputs do not fit {out_cap}")
            err.required = n.value
            raise err
        self._check(st, "adsb_decim_run_device")
        return n.value

    def demod_iq(self, iq, format: int = _lib.ADSB_DECIM_CS16, cap: Optional[int] = None) -> List[ModeSMessage]:
        """Host samples at factor x 2.4 MS/s of any length, in `format` (CS16, 8-bit, CF32: float32 or complex64, REAL16:
        1-D int16) -> the messages of the decimated stream (blocking)."""
        a = _as_format(iq, format)
        cap = cap or max(4096, a.shape[0] // (256 * self.factor))
        ptr = a.ctypes.data
        return self._ctx._collect(
            lambda out, c, n: self._L.adsb_decim_demod_iq(self._h, int(format), ptr, a.shape[0], out, c, n),
            "adsb_decim_demod_iq", cap)


def default_resampler_taps(up: int, down: int):
    """adsb_resamp_default_taps (host only): (taps int16[8 max(up, down) + 1], shift) of a Hamming-windowed sinc over the
    zero-stuffed rate with its cutoff at half the lower of the two rates."""
    L = _lib.lib()
    taps = np.zeros(8 * max(int(up), int(down), 1) + 1, dtype=np.int16)
    n, shift = C.c_uint32(), C.c_uint32()
    st = L.adsb_resamp_default_taps(int(up), int(down), taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size, C.byref(n),
                                    C.byref(shift))
    if st != _lib.ADSB_OK:
        raise AdsbError(st, f"adsb_resamp_default_taps: {L.adsb_strerror(st).decode()}")
    return taps[: n.value], int(shift.value)


def ratio_for_rate(rate_hz: int):
    """adsb_resamp_ratio_for_rate (host only): (up, down) that bring rate_hz to 2.4 MS/s.  AdsbError (ADSB_ERR_INVALID,
    with the terms in .ratio) where the ratio is outside what a resampler takes."""
    L = _lib.lib()
    up, down = C.c_uint32(), C.c_uint32()
    if not 0 < int(rate_hz) < 1 << 32:
        raise AdsbError(_lib.ADSB_ERR_INVALID, f"adsb_resamp_ratio_for_rate: {rate_hz} Hz")
    st = L.adsb_resamp_ratio_for_rate(int(rate_hz), C.byref(up), C.byref(down))
    if st != _lib.ADSB_OK:
        err = AdsbError(st, f"adsb_resamp_ratio_for_rate: {rate_hz} Hz needs {up.value}/{down.value}")
        err.ratio = (up.value, down.value)
        raise err
    return up.value, down.value


class Resampler:
    """One adsb_resamp: a stateful exact-integer polyphase FIR resampler by up / down on the context's device.  Close it
    before its context."""

    def __init__(self, ctx: Context, up: int, down: int, taps=None, shift: Optional[int] = None):
        self._ctx, self._L = ctx, ctx._L
        self._h = C.c_void_p()
        if taps is None:
            taps, default_shift = default_resampler_taps(up, down)
            shift = default_shift if shift is None else shift
        elif shift is None:
            raise ValueError("taps of the caller's need a shift")
        t = np.ascontiguousarray(taps, dtype=np.int16)
        if t.ndim != 1:
            raise ValueError("the taps are a flat int16 array")
        self.up, self.down, self.taps, self.shift = int(up), int(down), t, int(shift)
        self._check(self._L.adsb_resamp_create(ctx._h, int(up), int(down), t.ctypes.data, t.size, int(shift), C.byref(self._h)),
                    "adsb_resamp_create")

    def _check(self, st: int, what: str) -> None:
        self._ctx._check(st, what)

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            if self._ctx._h.value:   # (a context that is gone took the device state with it)
                self._L.adsb_resamp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self) -> None:
        self._check(self._L.adsb_resamp_reset(self._h), "adsb_resamp_reset")

    def set_mixer(self, table) -> None:
        """adsb_mix_set_resamp: the (period, 2) int16 table {c, s} the inputs consumed from now on are mixed with
        (None: no mixer)."""
        _set_mixer(self, self._L.adsb_mix_set_resamp, "adsb_mix_set_resamp", table)

    @property
    def mixer_period(self) -> int:
        return int(self._L.adsb_mix_get_resamp(self._h))

    def set_scale(self, scale: float) -> None:
        """adsb_fmt_set_scale_resamp: g of CF32 input, q(x) = clamp(rint(x g)); finite, 0 < g <= 2^31 (32768 by default)."""
        _set_scale(self, self._L.adsb_fmt_set_scale_resamp, "adsb_fmt_set_scale_resamp", scale)

    @property
    def scale(self) -> float:
        return float(self._L.adsb_fmt_get_scale_resamp(self._h))

    def set_input_stats(self, enabled: bool) -> None:
        """adsb_instat_set_resamp: opt-in; every input sample the resampler consumes from now on is counted on the device, raw,
        in front of the filter (input_stats()).  Disabling discards what was counted."""
        _set_input_stats(self, "resamp", enabled)

    @property
    def input_stats_enabled(self) -> bool:
        return int(self._L.adsb_instat_get_resamp(self._h)) == 1

    def input_stats(self) -> np.ndarray:
        """adsb_instat_fetch_resamp: waits for the handle's calls, then returns the record of the inputs consumed since the
        previous fetch (or the enable) as a 0-d structured array with the layout of adsb_input_stats, and zeroes it."""
        return _input_stats(self, "resamp")[0]

    def out_count(self, n_in: int) -> int:
        n = C.c_size_t()
        self._check(self._L.adsb_resamp_out_count(self._h, int(n_in), C.byref(n)), "adsb_resamp_out_count")
        return n.value

    def run_device(self, ptr_in: int, n_in: int, ptr_out: int, out_cap: int, format: int = _lib.ADSB_DECIM_CS16) -> int:
        """Device memory to device memory, enqueued without waiting; returns the output count.  AdsbError with status
        ADSB_ERR_CAPACITY (and the required count in .required) when out_cap is too small: nothing was consumed."""
        n = C.c_size_t()
        st = self._L.adsb_resamp_run_device(self._h, int(format), C.c_void_p(ptr_in), int(n_in), C.c_void_p(ptr_out), int(out_cap),
                                            C.byref(n))
        if st == _lib.ADSB_ERR_CAPACITY:
            err = AdsbError(st, f"adsb_resamp_run_device: {n.value} outputs do not fit {out_cap}")
            err.required = n.value
            raise err
        self._check(st, "adsb_resamp_run_device")
        return n.value

    def demod_iq(self, iq, format: int = _lib.ADSB_DECIM_CS16, cap: Optional[int] = None) -> List[ModeSMessage]:
        """Host samples at 2.4 MS/s x down / up of any length, in `format` (CS16, 8-bit, CF32: float32 or complex64,
        REAL16: 1-D int16) -> the messages of the resampled stream (blocking)."""
        a = _as_format(iq, format)
        cap = cap or max(4096, a.shape[0] * self.up // (256 * self.down))
        ptr = a.ctypes.data
        return self._ctx._collect(
            lambda out, c, n: self._L.adsb_resamp_demod_iq(self._h, int(format), ptr, a.shape[0], out, c, n),
            "adsb_resamp_demod_iq", cap)


class ResamplerBank:
    """One adsb_bank: n_streams stateful resampler streams of one ratio and one filter on the context's device, advanced
    by one call (include/adsb_hip.h, "Resampler banks").  Close it before its context."""

    ALL = 0xFFFFFFFF   # ADSB_BANK_ALL

    def __init__(self, ctx: Context, n_streams: int, up: int, down: int, taps=None, shift: Optional[int] = None):
        self._ctx, self._L = ctx, ctx._L
        self._h = C.c_void_p()
        if taps is None:
            taps, default_shift = default_resampler_taps(up, down)
            shift = default_shift if shift is None else shift
        elif shift is None:
            raise ValueError("taps of the caller's need a shift")
        t = np.ascontiguousarray(taps, dtype=np.int16)
        if t.ndim != 1:
            raise ValueError("the taps are a flat int16 array")
        self.up, self.down, self.taps, self.shift = int(up), int(down), t, int(shift)
        self._check(self._L.adsb_bank_create(ctx._h, int(n_streams), int(up), int(down), t.ctypes.data, t.size, int(shift),
                                             C.byref(self._h)), "adsb_bank_create")

    def _check(self, st: int, what: str) -> None:
        self._ctx._check(st, what)

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            if self._ctx._h.value:   # (a context that is gone took the device state with it)
                self._L.adsb_bank_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def streams(self) -> int:
        return int(self._L.adsb_bank_streams(self._h))

    def reset(self, stream: Optional[int] = None) -> None:
        """One stream, or every stream (None), starts over: P = 0 and a zero history, ordered on the stream like a run."""
        self._check(self._L.adsb_bank_reset(self._h, self.ALL if stream is None else int(stream)), "adsb_bank_reset")

    def consumed(self, stream: int) -> int:
        p = C.c_uint64()
        self._check(self._L.adsb_bank_consumed(self._h, int(stream), C.byref(p)), "adsb_bank_consumed")
        return p.value

    def out_count(self, stream: int, n_in: int) -> int:
        n = C.c_size_t()
        self._check(self._L.adsb_bank_out_count(self._h, int(stream), int(n_in), C.byref(n)), "adsb_bank_out_count")
        return n.value

    def inputs_for(self, stream: int, n_out: int):
        """(n_in, n_out_made): the fewest inputs behind the stream's P that give at least n_out outputs, and how many they
        give (n_out, or one more where up > down)."""
        n_in, made = C.c_size_t(), C.c_size_t()
        self._check(self._L.adsb_bank_inputs_for(self._h, int(stream), int(n_out), C.byref(n_in), C.byref(made)),
                    "adsb_bank_inputs_for")
        return n_in.value, made.value

    def run_device(self, streams, ptrs_in, n_in, ptrs_out, out_caps, format: int = _lib.ADSB_DECIM_CS16) -> np.ndarray:
        """Run r advances streams[r] by n_in[r] inputs at device address ptrs_in[r] and writes its outputs to ptrs_out[r]
        (room for out_caps[r]); one launch for all of them, enqueued without waiting.  Returns the output counts.
        AdsbError with status ADSB_ERR_CAPACITY (and the required counts in .required) when a run does not fit: nothing
        was consumed."""
        s = np.ascontiguousarray(streams, dtype=np.uint32)
        pi, po = np.ascontiguousarray(ptrs_in, dtype=np.uintp), np.ascontiguousarray(ptrs_out, dtype=np.uintp)
        ni, caps = np.ascontiguousarray(n_in, dtype=np.uintp), np.ascontiguousarray(out_caps, dtype=np.uintp)
        if not (s.ndim == 1 and s.shape == pi.shape == po.shape == ni.shape == caps.shape):
            raise ValueError("streams, pointers, counts and capacities are flat arrays of one length")
        n = np.zeros(max(s.size, 1), dtype=np.uintp)
        st = self._L.adsb_bank_run_device(self._h, int(format), s.size, s.ctypes.data, pi.ctypes.data, ni.ctypes.data,
                                          po.ctypes.data, caps.ctypes.data, n.ctypes.data)
        n = n[: s.size]
        if st == _lib.ADSB_ERR_CAPACITY:
            err = AdsbError(st, f"adsb_bank_run_device: {n.tolist()} outputs do not fit {caps.tolist()}")
            err.required = n
            raise err
        self._check(st, "adsb_bank_run_device")
        return n

    def set_mixer(self, table) -> None:
        """adsb_bank_set_mixer: the (period, 2) int16 table {c, s} every stream's inputs consumed from now on are mixed
        with, each stream at its own phase (None: no mixer)."""
        _set_mixer(self, self._L.adsb_bank_set_mixer, "adsb_bank_set_mixer", table)

    @property
    def mixer_period(self) -> int:
        return int(self._L.adsb_bank_get_mixer(self._h))

    def set_scale(self, scale: float) -> None:
        """adsb_bank_set_scale: g of CF32 input, q(x) = clamp(rint(x g)); finite, 0 < g <= 2^31 (32768 by default)."""
        _set_scale(self, self._L.adsb_bank_set_scale, "adsb_bank_set_scale", scale)

    @property
    def scale(self) -> float:
        return float(self._L.adsb_bank_get_scale(self._h))

    def set_input_stats(self, enabled: bool) -> None:
        """adsb_instat_set_bank: opt-in; every input sample any stream of the bank consumes from now on is counted on the device, raw,
        in front of the filter (input_stats()).  Disabling discards what was counted."""
        _set_input_stats(self, "bank", enabled)

    @property
    def input_stats_enabled(self) -> bool:
        return int(self._L.adsb_instat_get_bank(self._h)) == 1

    def input_stats(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """adsb_instat_fetch_bank: waits for the bank's calls, then returns the records of streams first .. first + n - 1
        (n = None: up to the last) over the inputs each consumed since its previous fetch (or the enable), as a structured
        array with the layout of adsb_input_stats, and zeroes exactly those."""
        return _input_stats(self, "bank", first, self.streams - int(first) if n is None else n)


_default: Optional[Context] = None


def default_context() -> Context:
    """The process-wide context that stands in for the reference's global filter
    statics (src/icao_filter.rs:8-9).  Device = LOCAL_RANK if set, else 0."""
    global _default
    if _default is None:
        _default = Context(device=int(os.environ.get("LOCAL_RANK", "0")), max_chunks=1)
    return _default
