"""Shared by the tests of receiver seams scored on the device (include/adsb_hip.h, "Receiver seams, scored on the device":
tests/test_gpu_receiver_seams_scored.py): dense passes of 20 buffers whose buffers belong to several receivers, with seam
frames planted across the end of a receiver's buffer and the start of its next one -- wherever in the call, or in a later
call, that next buffer is -- and the expectation the header defines: tests/seam_support.py's SeamModel, one CPU oracle with
carry-over per receiver.  Two more expectations are computed from the same input, so that a test can assert on the CPU
what its input is for before the GPU is touched: the same receivers without carry (the planted seam frames are not found)
and with carry but ONE shared filter (a different list).

The dense input is F.fill_capture(seed, n, per_buffer=60): its frames start at samples 200 .. CHUNK - 420 of a buffer, so
the last 220 and the first 200 samples of every buffer are noise, and that is where the seam frames go."""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from dump1090_rs_amd import synth
from tests import formats_support as F
from tests import receivers_support as RS
from tests import seam_support as S

CHUNK, LEAD = S.CHUNK, S.LEAD
N = 20
WINDOW = 700   # samples on either side of a seam a planted frame may touch


@lru_cache(maxsize=None)
def dense(seed: int = 900, n: int = N, per_buffer: int = 60) -> np.ndarray:
    iq = F.fill_capture(seed, n, per_buffer=per_buffer)
    iq.setflags(write=False)
    return iq


class SharedFilterModel(S.SeamModel):
    """SeamModel with every receiver's carry its own and ONE filter for all: what an implementation that shares a filter
    across receivers would compute."""

    def __init__(self, n: int, mode: int = 0):
        super().__init__(n, mode, True)
        if mode == 0:
            self.streams = [self.streams[0]] * n
        self._share()

    def _share(self):
        if self.mode:
            for s in self.streams[1:]:
                s.filter = self.streams[0].filter

    def flush(self, r: Optional[int] = None) -> None:
        super().flush(None)   # (one filter: a flush of one receiver is a flush of all)
        self._share()


def plant(prev_iq: np.ndarray, prev_b: int, iq: np.ndarray, b: int, at: int, frame: bytes, tick: int = 0, amplitude: int = 24000,
          angle: int = 1, loud: bool = False) -> None:
    """`frame` with its first preamble pulse at sample `at` of buffer b of `iq` (negative: that many samples before the end
    of buffer prev_b of `prev_iq`, the buffer in front of it in its receiver's stream).  loud: the sample in front of
    buffer b is full scale."""
    pa, a = (prev_b + 1) * CHUNK - WINDOW, b * CHUNK
    scratch = np.concatenate([prev_iq[pa:pa + WINDOW], iq[a:a + WINDOW]])
    synth.add_bursts(scratch, [synth.Burst(5 * (WINDOW + at) + tick, amplitude, angle, frame)])
    prev_iq[pa:pa + WINDOW] = scratch[:WINDOW]
    iq[a:a + WINDOW] = scratch[WINDOW:]
    if loud:
        prev_iq[(prev_b + 1) * CHUNK - 1] = (32000, 0)


KINDS = ("straddle", "inside", "last", "edge")


def seam_passes(maps: Sequence[np.ndarray], seed: int = 900, every: int = 3, kinds: Sequence[str] = KINDS):
    """One input per map -- the dense capture's first len(map) buffers -- with a frame planted at every `every`-th seam, a
    seam being a buffer whose receiver has an earlier buffer in this or an earlier pass; the kinds of S.catalogue in
    rotation.  -> (inputs, {kind: [(pass, buffer, receiver, frame)]})"""
    inputs = [dense(seed)[:len(m) * CHUNK].copy() for m in maps]
    latest: Dict[int, Tuple[int, int]] = {}
    planted = {k: [] for k in KINDS}
    seams = 0
    for k, m in enumerate(maps):
        for b, r in enumerate(int(x) for x in m):
            if r in latest:
                if seams % every == 0:
                    n = seams // every
                    kind = kinds[n % len(kinds)]
                    pk, pb = latest[r]
                    addr = 0x480000 + 0x111 * n + r
                    if kind == "straddle":
                        f = synth.df17_frame(addr, 0x58B986D0B3BD25 + n)
                        plant(inputs[pk], pb, inputs[k], b, -100, f, n % 5, F.AMPLITUDES[n % 5], n % 16)
                    elif kind == "inside":
                        f = synth.df11_frame(addr)
                        plant(inputs[pk], pb, inputs[k], b, -190, f, n % 5, F.AMPLITUDES[n % 5], n % 16)
                    elif kind == "last":
                        f = synth.df17_frame(addr, 0x99AA5511223344 + n)
                        plant(inputs[pk], pb, inputs[k], b, -1, f, n % 5, F.AMPLITUDES[n % 5], n % 16)
                    else:
                        f = synth.df17_frame(addr, 0x2233445566778 + n)
                        plant(inputs[pk], pb, inputs[k], b, 0, f, 0, F.AMPLITUDES[n % 5], n % 16, loud=True)
                    planted[kind].append((k, b, r, f))
                seams += 1
            latest[r] = (k, b)
    return inputs, planted


def expect(n_receivers: int, calls: Sequence[Tuple[np.ndarray, Sequence[int]]], mode: int = 0, before: Optional[Dict[int, list]] = None):
    """calls: (iq, map) per pass.  before: {pass: [("flush" | "reset", receiver or None)]}.
    -> (lists with carry and a filter per receiver, the same without carry, with carry and one shared filter, the model)"""
    own, without, shared = S.SeamModel(n_receivers, mode), S.SeamModel(n_receivers, mode, carry=False), SharedFilterModel(n_receivers, mode)
    wants, withouts, shareds = [], [], []
    for k, (iq, m) in enumerate(calls):
        for what, r in (before or {}).get(k, []):
            for model in (own, without, shared):
                model.flush(r) if what == "flush" else model.reset(r)
        wants.append(own.feed(iq, m))
        withouts.append(without.feed(iq, m))
        shareds.append(shared.feed(iq, m))
    return wants, withouts, shareds, own


def assert_input_is_for_this(n_receivers: int, calls, wants, withouts, shareds, seam_frames: Sequence[bytes]) -> None:
    """What every parity test asserts on the CPU before the GPU is touched: the planted seam frames are found with carry
    and not without; one shared filter would give a different list; every pass is dense -- at least 8 messages, so at least
    8 trial records, per buffer."""
    S.assert_seams_matter(sum(wants, []), sum(withouts, []), seam_frames)
    RS.assert_tells_apart(n_receivers, sum(wants, []), sum(shareds, []))
    for (iq, m), want in zip(calls, wants):
        assert len(want) >= 8 * len(m), (len(want), len(m))


def seam_frames_of(planted) -> List[bytes]:
    return [f for kind in ("straddle", "inside") for _, _, _, f in planted[kind]]
