"""Shared by the tests of receiver seams (include/adsb_hip.h, "Receiver seams": tests/test_receiver_seams_cpu.py,
tests/test_gpu_receiver_seams.py): per-receiver sample streams with frames planted across the ends of their buffers, the
interleaving of those streams into the buffers of one call, and the expectation the header defines -- one CPU oracle
WITH CARRY-OVER per receiver (oracle.binding.demod_iq_carry; under a repair mode the restatement with carry=True), one
call per buffer, every message relabelled with the buffer's index, merged in (chunk, j) order.  The same input without
carry is computed too: a test first asserts on the CPU that its planted seam frames are found with carry and not
without."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from dump1090_rs_amd import synth
from tests import formats_support as F
from tests import receivers_support as RS

CHUNK, LEAD = RS.CHUNK, 326


# ------------------------------------------------------------------------------------------------------ the model
class SeamModel:
    """n independent streams of the reference with carry-over on the CPU."""

    def __init__(self, n: int, mode: int = 0, carry: bool = True):
        self.mode, self.carry_on = mode, carry
        self.streams = [self._new() for _ in range(n)]
        self.carry = [np.zeros((LEAD, 2), dtype=np.int16) for _ in range(n)]

    def _new(self):
        if self.mode == 0:
            from oracle import binding
            return binding.Oracle()
        if self.mode == 1:
            from tests import fix_support
            return fix_support.Restated(1, carry=self.carry_on)
        from tests import fix2_support
        return fix2_support.Restated(3, carry=self.carry_on)

    def flush(self, r: Optional[int] = None) -> None:
        for s in (self.streams if r is None else [self.streams[r]]):
            s.icao_flush()

    def reset(self, r: Optional[int] = None) -> None:
        """adsb_receiver_carry_reset: nothing precedes the next buffer of receiver r (None: of every receiver)"""
        for k in (range(len(self.streams)) if r is None else [r]):
            self.carry[k][:] = 0
            if self.mode and self.streams[k].carry is not None:
                self.streams[k].carry[:] = 0

    def table(self, r: int) -> List[int]:
        return list(self.streams[r].filter.a)

    def feed(self, iq: np.ndarray, receivers: Sequence[int]) -> List[tuple]:
        """One call: buffer b of `iq` through receiver receivers[b]'s stream, its messages relabelled with b."""
        from oracle import binding
        out = []
        for b, a in enumerate(range(0, len(iq), CHUNK)):
            r = int(receivers[b])
            s = self.streams[r]
            part = np.ascontiguousarray(iq[a:a + CHUNK])
            if self.mode:
                out += [RS._rkey(k, b) for k in s.demod_iq(part)]
            elif self.carry_on:
                out += [RS._okey(w, b) for w in binding.demod_iq_carry(s, part, self.carry[r], cap=1 << 16)[0]]
            else:
                out += [RS._okey(w, b) for w in s.demod_iq(part, cap=1 << 16)[0]]
        return out


def tables_equal(c, model: SeamModel, n_receivers: int) -> None:
    for r in range(n_receivers):
        assert list(c.receiver_filter_table(r)) == model.table(r), r


# ------------------------------------------------------------------------------------------------------ the input
Plant = Tuple[int, bytes, int]   # (sample of the receiver's stream at which the first preamble pulse starts, frame, sub-sample tick)


def stream(seed: int, n_buffers: int, plants: Sequence[Plant], short: int = 0, loud_before: Sequence[int] = ()) -> np.ndarray:
    """One receiver's samples: n_buffers buffers of noise (`short`: that many samples cut off the end), the planted
    frames, and at every sample of `loud_before` a full-scale sample (what makes data[j] >= data[j + 1] for the frame
    that starts right behind it)."""
    iq = synth.noise_numpy(n_buffers * CHUNK - short, seed)
    synth.add_bursts(iq, [synth.Burst(5 * at + tick, F.AMPLITUDES[k % len(F.AMPLITUDES)], (3 * k + 1) % 16, frame)
                          for k, (at, frame, tick) in enumerate(plants)])
    for s in loud_before:
        iq[s] = (32000, 0)
    return iq


def interleave(streams: Sequence[np.ndarray], receivers: Sequence[int]) -> np.ndarray:
    """Buffer b of the result is the next unused buffer (the last may be short) of streams[receivers[b]]."""
    used = [0] * len(streams)
    parts = []
    for r in receivers:
        r = int(r)
        parts.append(streams[r][used[r] * CHUNK:(used[r] + 1) * CHUNK])
        used[r] += 1
    return np.ascontiguousarray(np.concatenate(parts))


def aircraft(r: int, k: int) -> int:
    return 0x480000 + 0x1111 * r + 0x10 * k + 1


def catalogue(n_receivers: int = 3, per: int = 4, seed: int = 900):
    """Per receiver `per` buffers; across the end of buffer k of receiver r (k < per - 1), in rotation:
      0  a DF17 that starts 100 samples before the end, and a DF11 wholly inside the last 326 samples
      1  a DF17 that starts at the very last sample
      2  a DF17 whose first preamble pulse is sample 0 of the next buffer, behind a full-scale last sample: a zero
         lead-in finds it at j = 325, the real one does not
    -> (streams, {kind: [(receiver, the frame's bytes)]})."""
    streams, planted = [], {"straddle": [], "inside": [], "last": [], "edge": []}
    for r in range(n_receivers):
        plants, loud = [], []
        for k in range(per - 1):
            end = (k + 1) * CHUNK
            kind = (k + r) % 3
            if kind == 0:
                a, b = synth.df17_frame(aircraft(r, 2 * k), 0x58B986D0B3BD25 + k), synth.df11_frame(aircraft(r, 2 * k + 1))
                plants += [(end - 300, b, (r + k) % 5), (end - 100, a, (2 * r + k) % 5)]
                planted["inside"].append((r, b))
                planted["straddle"].append((r, a))
            elif kind == 1:
                a = synth.df17_frame(aircraft(r, 2 * k), 0x99AA5511223344 + k)
                plants.append((end - 1, a, (r + 2 * k) % 5))
                planted["last"].append((r, a))
            else:
                a = synth.df17_frame(aircraft(r, 2 * k), 0x2233445566778 + k)
                plants.append((end, a, 0))
                loud.append(end - 1)
                planted["edge"].append((r, a))
        streams.append(stream(seed + r, per, plants, loud_before=loud))
    return streams, planted


def round_robin(n_receivers: int, per: int) -> np.ndarray:
    return np.tile(np.arange(n_receivers, dtype=np.uint32), per)


def found(keys_: List[tuple], frame: bytes) -> List[tuple]:
    """(chunk, j, score) of every emission of `frame`"""
    return [(k[0], k[1], k[3]) for k in keys_ if k[4] == frame[:k[5]] and k[5] == len(frame)]


def expect_calls(n_receivers: int, calls: Sequence[Tuple[np.ndarray, Sequence[int]]], mode: int = 0, carry: bool = True,
                 before: Optional[Dict[int, list]] = None):
    """calls: (iq, map) per call / pass.  before: {call: [("flush" | "reset", receiver or None)]} applied in front of
    it.  -> (a list of keys per call, the model)"""
    model = SeamModel(n_receivers, mode, carry)
    out = []
    for k, (iq, m) in enumerate(calls):
        for what, r in (before or {}).get(k, []):
            model.flush(r) if what == "flush" else model.reset(r)
        out.append(model.feed(iq, m))
    return out, model


def assert_seams_matter(with_carry: List[tuple], without: List[tuple], seam_frames: Sequence[bytes]) -> None:
    """What every GPU test asserts first, on the CPU: the oracle with carry finds every planted seam frame, the oracle
    without finds none of them."""
    for f in seam_frames:
        assert found(with_carry, f), f.hex()
        assert not found(without, f), f.hex()
