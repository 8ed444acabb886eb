"""Shared by the tests of "many receivers, one pass" (tests/test_receivers_cpu.py, tests/test_gpu_receivers.py,
tests/fuzz_gpu_receivers.py): captures of several receivers that share aircraft, interleaved buffer by buffer by a seeded
map, and the expectation the header defines -- one CPU oracle per receiver, one demod_iq per buffer, every message
relabelled with the buffer's index in the call.  The same input under ONE shared filter is computed too: a parity test
first asserts that the two expectations differ, so that it would fail on an implementation that shares a filter."""
from __future__ import annotations

import struct
from functools import lru_cache
from typing import List, Optional, Sequence

import numpy as np

from tests import formats_support as F

CHUNK = F.CHUNK


# ------------------------------------------------------------------------------------------------------ keys
def key_of(chunk, j, try_phase, score, msg: bytes, length, signal_level) -> tuple:
    """(chunk, j, try_phase, score, msg, len, the bits of signal_level)"""
    return (int(chunk), int(j), int(try_phase), int(score), bytes(msg[:length]), int(length), struct.pack("<d", float(signal_level)))


def keys(msgs) -> List[tuple]:
    """... of the library's messages (ModeSMessage)"""
    return [key_of(m.chunk, m.j, m.try_phase, m.score, m.msg, m.msglen, m.signal_level) for m in msgs]


def _okey(w: dict, chunk: int) -> tuple:
    return key_of(chunk, w["j"], w["try_phase"], w["score"], w["msg"], w["len"], w["signal_level"])


def _rkey(k: tuple, chunk: int) -> tuple:
    """from fix_support.okey: (buffer bytes, score, j, try_phase, chunk, signal_level)"""
    return key_of(chunk, k[2], k[3], k[1], k[0], len(k[0]), k[5])


# ------------------------------------------------------------------------------------------------------ the model
class Model:
    """n independent streams of the reference on the CPU: the oracle, or under an error-correction mode its restatement
    (tests/fix_support.py, tests/fix2_support.py).  shared=True: every receiver is the same stream -- what an
    implementation with one filter for all would compute."""

    def __init__(self, n: int, mode: int = 0, shared: bool = False):
        self.mode = mode
        one = self._new() if shared else None
        self.streams = [one if shared else self._new() for _ in range(n)]

    def _new(self):
        if self.mode == 0:
            from oracle import binding
            return binding.Oracle()
        if self.mode == 1:
            from tests import fix_support
            return fix_support.Restated(1)
        from tests import fix2_support
        return fix2_support.Restated(3)

    def flush(self, r: Optional[int] = None) -> None:
        for s in (self.streams if r is None else [self.streams[r]]):
            s.icao_flush()

    def table(self, r: int) -> List[int]:
        return list(self.streams[r].filter.a)

    def feed(self, iq: np.ndarray, receivers: Sequence[int]) -> List[tuple]:
        """One call: buffer b of `iq` through receiver receivers[b]'s stream, its messages relabelled with b."""
        out = []
        for b, a in enumerate(range(0, len(iq), CHUNK)):
            s = self.streams[int(receivers[b])]
            part = np.ascontiguousarray(iq[a:a + CHUNK])
            if self.mode == 0:
                out += [_okey(w, b) for w in s.demod_iq(part, cap=1 << 16)[0]]
            else:
                out += [_rkey(k, b) for k in s.demod_iq(part)]
        return out


# ------------------------------------------------------------------------------------------------------ the input
@lru_cache(maxsize=None)
def receiver_capture(seed: int, n_buffers: int, first_pass: int, fix: bool = False, cross_seed: int = 5) -> np.ndarray:
    """One receiver's capture: every class of the formats stream in every buffer, and the cross_pass aircraft -- the
    same ones for every receiver (one cross_pass seed), heard in a different order by each (first_pass)."""
    iq = F.formats_capture(seed, n_buffers, fix=fix, edges=False, extra=F.cross_pass(3, 2, seed=cross_seed, first_pass=first_pass))[0]
    iq.setflags(write=False)
    return iq


def seeded_map(n_receivers: int, per: int, seed: int) -> np.ndarray:
    m = np.repeat(np.arange(n_receivers, dtype=np.uint32), per)
    np.random.default_rng([0x5EED, seed]).shuffle(m)
    return m


def interleave(captures: Sequence[np.ndarray], receivers: Sequence[int]) -> np.ndarray:
    """Buffer b of the result is the next unused buffer of captures[receivers[b]]."""
    used = [0] * len(captures)
    parts = []
    for r in receivers:
        r = int(r)
        parts.append(captures[r][used[r] * CHUNK:(used[r] + 1) * CHUNK])
        used[r] += 1
    return np.ascontiguousarray(np.concatenate(parts))


@lru_cache(maxsize=None)
def batch(n_receivers: int, per: int, seed0: int = 10, map_seed: int = 1, fix: bool = False):
    """(iq, map) of n_receivers captures of `per` buffers each (seeds seed0 ..), interleaved by a seeded shuffle.
    batch(3, 6) is the 18-buffer input whose two expectations differ by 30 / 26 messages and 10 scores."""
    caps = [receiver_capture(seed0 + r, per, r, fix) for r in range(n_receivers)]
    m = seeded_map(n_receivers, per, map_seed)
    iq = interleave(caps, m)
    iq.setflags(write=False)
    m.setflags(write=False)
    return iq, m


@lru_cache(maxsize=None)
def expectations(n_receivers: int, per: int, seed0: int = 10, map_seed: int = 1, fix: bool = False, mode: int = 0):
    """(per-receiver expectation, shared-filter expectation, the per-receiver model after the call) of batch(...) as ONE
    call from empty filters."""
    iq, m = batch(n_receivers, per, seed0, map_seed, fix)
    own, shared = Model(n_receivers, mode), Model(n_receivers, mode, shared=True)
    return own.feed(iq, m), shared.feed(iq, m), own


def differ(want: List[tuple], shared: List[tuple]) -> tuple:
    """(messages only under the shared filter, only with per-receiver filters, positions that carry a different score)"""
    a, b = {k[:2]: k for k in shared}, {k[:2]: k for k in want}
    return (len(set(shared) - set(want)), len(set(want) - set(shared)), sum(a[p][3] != b[p][3] for p in set(a) & set(b)))


def assert_tells_apart(n_receivers: int, want: List[tuple], shared: List[tuple]) -> None:
    """What every parity test asserts first: with more than one receiver its input gives a different list under one
    shared filter (with one receiver the two are the same thing)."""
    if n_receivers > 1:
        only_shared, only_own, rescored = differ(want, shared)
        assert want != shared and only_shared + only_own + rescored > 0, (only_shared, only_own, rescored)
    else:
        assert want == shared


# ------------------------------------------------------------------------------------------------------ trial records
def trial_records(iq: np.ndarray) -> np.ndarray:
    """The oracle's trial records of every buffer of `iq` (oracle.binding.all_trials), chunk = buffer index."""
    from oracle import binding
    parts = [binding.all_trials(np.ascontiguousarray(iq[a:a + CHUNK]), chunk=b)[1] for b, a in enumerate(range(0, len(iq), CHUNK))]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=binding.TRIAL_DTYPE)
