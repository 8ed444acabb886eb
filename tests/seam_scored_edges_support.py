"""Shared by tests/test_gpu_receiver_seams_scored_edges.py and tests/test_receiver_seams_scored_edges_cpu.py: the inputs
that take the device-side seam merge (csrc/adsb_seam_score.hip) and the keyed score kernels (csrc/adsb_score_rx.hip) where
the 20-buffer, five-receiver shape of tests/test_gpu_receiver_seams_scored.py never goes, and what each input is for,
asserted on the CPU while it is built:

  leg A   passes of 256 / 257 / 260 buffers in a context of 260: k_seam_prefix's second block of buffers and its carry
  leg B   receiver indices above 8 and above 12 bits, out of 16384: rx_key, the first-adder entry, the carry rows
  leg C   buffers without an own hit inside an ordered pass (k_seam_mark's three fills of own_start), and a pass that is
          nothing but seam records
  leg D   an own hit dropped in buffer 0 with no seam record before buffer 8: own_shift below zero from the start

The expectation is tests/seam_support.py's SeamModel, as everywhere; every builder is cached, so the GPU file pays for a
case once whether or not the CPU file has run before it."""
from __future__ import annotations

from functools import lru_cache
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from dump1090_rs_amd import synth
from tests import formats_support as F
from tests import receivers_support as RS
from tests import seam_support as S
from tests import seam_scored_support as SS

CHUNK, LEAD, N = SS.CHUNK, SS.LEAD, SS.N
X = 0x4B1A2C
DF17_X = synth.df17_frame(X, 0x58B986D0B3BD25)
REPLY_X = F.ap_frame(4, X, 0x1234567)
REPLY_X2 = F.ap_frame(4, X, 0x0765432)
SEAM_KINDS = ("straddle", "inside")   # the kinds that are found with carry and not without


# ------------------------------------------------------------------------------------------------- planting
def plant_kind(prev_iq: np.ndarray, prev_b: int, iq: np.ndarray, b: int, kind: str, n: int) -> bytes:
    """The n-th planted frame, of `kind`, across the end of buffer prev_b of prev_iq and the start of buffer b of iq: what
    SS.seam_passes plants, with an address of its own per frame."""
    addr = 0x480001 + 3 * n
    amplitude, angle = F.AMPLITUDES[n % 5], n % 16
    if kind == "straddle":
        f = synth.df17_frame(addr, 0x58B986D0B3BD25 + n)
        SS.plant(prev_iq, prev_b, iq, b, -100, f, n % 5, amplitude, angle)
    elif kind == "inside":
        f = synth.df11_frame(addr)
        SS.plant(prev_iq, prev_b, iq, b, -190, f, n % 5, amplitude, angle)
    elif kind == "last":
        f = synth.df17_frame(addr, 0x99AA5511223344 + n)
        SS.plant(prev_iq, prev_b, iq, b, -1, f, n % 5, amplitude, angle)
    else:
        f = synth.df17_frame(addr, 0x2233445566778 + n)
        SS.plant(prev_iq, prev_b, iq, b, 0, f, 0, amplitude, angle, loud=True)
    return f


def plant_seams(inputs: Sequence[np.ndarray], maps: Sequence[np.ndarray], every: int = 3, kinds: Sequence[str] = SS.KINDS,
                skip: Optional[Callable[[int, int], bool]] = None, force: Optional[Dict[Tuple[int, int], str]] = None, first: int = 0):
    """SS.seam_passes over inputs of the caller's: a frame at every `every`-th seam, the kinds in rotation.  skip(pass,
    buffer): no frame in front of that buffer; force[(pass, buffer)]: this kind there, outside the rotation.
    -> {kind: [(pass, buffer, receiver, frame)]}"""
    latest: Dict[int, Tuple[int, int]] = {}
    planted = {k: [] for k in SS.KINDS}
    seams = rotation = 0
    n = first
    for k, m in enumerate(maps):
        for b, r in enumerate(int(x) for x in m):
            if r in latest and not (skip and skip(k, b)):
                kind = (force or {}).get((k, b))
                if kind is None:
                    if seams % every == 0:
                        kind = kinds[rotation % len(kinds)]
                        rotation += 1
                    seams += 1
                if kind:
                    pk, pb = latest[r]
                    planted[kind].append((k, b, r, plant_kind(inputs[pk], pb, inputs[k], b, kind, n)))
                    n += 1
            latest[r] = (k, b)
    return planted


def previous(maps: Sequence[Sequence[int]], k: int, b: int) -> Tuple[int, int]:
    """(pass, buffer) of the buffer in front of buffer b of pass k in its receiver's stream"""
    r = int(maps[k][b])
    for pk in range(k, -1, -1):
        for pb in range(b - 1 if pk == k else len(maps[pk]) - 1, -1, -1):
            if int(maps[pk][pb]) == r:
                return pk, pb
    raise AssertionError((k, b, r))


def plant_at(inputs, maps, k: int, b: int, at: int, frame: bytes, n: int = 0, loud: bool = False) -> None:
    pk, pb = previous(maps, k, b)
    SS.plant(inputs[pk], pb, inputs[k], b, at, frame, n % 5, F.AMPLITUDES[n % 5], n % 16, loud=loud)


def teach(iq: np.ndarray, b: int, frame: bytes, k: int = 0, j: int = 40000) -> None:
    """`frame` alone in 600 samples of fresh noise in the middle of buffer b"""
    a = b * CHUNK + j
    iq[a - 100:a + 500] = synth.noise_numpy(600, seed=4242 + k)
    synth.add_bursts(iq, [synth.Burst(5 * a + 1, 24000, 2, frame)])


def silence(iq: np.ndarray, buffers: Sequence[int]) -> None:
    """all-zero IQ: magnitude 0 everywhere fails every strict comparison of the preamble test, so not one own hit"""
    for b in buffers:
        iq[b * CHUNK:(b + 1) * CHUNK] = 0


def is_silent(iq: np.ndarray, b: int) -> bool:
    return not iq[b * CHUNK:(b + 1) * CHUNK].any()


def in_buffer(keys: List[tuple], b: int) -> List[tuple]:
    return [k for k in keys if k[0] == b]


def emissions(keys: List[tuple], frame: bytes) -> List[tuple]:
    """(buffer, found across the seam, score) of every emission of `frame`"""
    return sorted({(c, j < LEAD, score) for c, j, score in S.found(keys, frame)})


def seam_frames(planted, kinds: Sequence[str] = SEAM_KINDS) -> List[Tuple[int, int, bytes]]:
    return [(k, b, f) for kind in kinds for k, b, _, f in planted[kind]]


def found_at_the_seam(wants: Sequence[List[tuple]], k: int, b: int, f: bytes) -> bool:
    return any(c == b and j < LEAD for c, j, _ in S.found(wants[k], f))


def assert_dense(wants: Sequence[List[tuple]], maps: Sequence[Sequence[int]], passes: Optional[Sequence[int]] = None) -> None:
    for k in (range(len(maps)) if passes is None else passes):
        assert len(wants[k]) >= 8 * len(maps[k]), (k, len(wants[k]))


def assert_seams_found(wants, withouts, planted, missing: int = 0) -> List[Tuple[int, int, bytes]]:
    """The planted straddling and inside frames the model finds at their seam -- all of them but `missing` at the most --
    and S.assert_seams_matter over those: found with carry, not without."""
    frames = seam_frames(planted)
    found = [(k, b, f) for k, b, f in frames if found_at_the_seam(wants, k, b, f)]
    assert frames and len(found) >= len(frames) - missing, (len(found), len(frames))
    S.assert_seams_matter(sum(wants, []), sum(withouts, []), [f for _, _, f in found])
    return found


def feed_all(model, inputs, maps) -> List[List[tuple]]:
    return [model.feed(iq, m) for iq, m in zip(inputs, maps)]


# ------------------------------------------------------------------------------------------------- leg A
A_CONTEXT, A_RECEIVERS, A_BLOCK = 260, 6, 256   # (A_BLOCK: k_seam_prefix scans this many buffers a turn)


def tiled(n: int) -> np.ndarray:
    """SS.dense() repeated to n buffers (np.tile: 30 ms for 260 buffers, where 260 fresh ones take 8 s)"""
    return np.tile(SS.dense(), (-(-n // N), 1))[:n * CHUNK]


def leg_a_maps(nb: int) -> List[np.ndarray]:
    r = np.random.default_rng([0x5EA3, 0xA, nb])
    return [r.integers(0, A_RECEIVERS, size=nb).astype(np.uint32) for _ in range(2)]


def leg_a_inputs(nb: int):
    """Two passes of nb tiled buffers, the four kinds planted in rotation at every third seam; behind the first block a
    seam frame is planted in front of buffer 256 of the first pass and an edge frame in front of buffer 256 of the second.
    Not cached (136 MB a pass): built again wherever it is needed, in 0.2 s.  -> (inputs, maps, planted)"""
    maps = leg_a_maps(nb)
    inputs = [tiled(nb), tiled(nb)]
    force = {(0, A_BLOCK): "straddle", (1, A_BLOCK): "edge"} if nb > A_BLOCK else {}
    return inputs, maps, plant_seams(inputs, maps, force=force)


@lru_cache(maxsize=None)
def leg_a_case(nb: int):
    """-> (maps, the model's lists, the model, planted)"""
    inputs, maps, planted = leg_a_inputs(nb)
    own, without = S.SeamModel(A_RECEIVERS), S.SeamModel(A_RECEIVERS, carry=False)
    wants, withouts = feed_all(own, inputs, maps), feed_all(without, inputs, maps)
    found = assert_seams_found(wants, withouts, planted, missing=len(seam_frames(planted)) // 20)
    assert any(b < A_BLOCK for _, b, _ in found)
    assert_dense(wants, maps)
    # no table comes near the point where the host takes a pass back (held + distinct additions + 64 < 4096): the tiled
    # capture repeats its aircraft, so a receiver hears thousands of DF17 / DF18 frames of a few hundred addresses
    assert all(sum(a != 0 for a in own.table(r)) < 4096 - 64 - 1024 for r in range(A_RECEIVERS))
    if nb > A_BLOCK:
        assert any(b >= A_BLOCK for _, b, _ in found)
        # the seam frame in front of buffer 256 of the first pass: found there; its receiver's previous buffer is in the first block
        (f,) = [f for k, b, _, f in planted["straddle"] if (k, b) == (0, A_BLOCK)]
        assert found_at_the_seam(wants, 0, A_BLOCK, f) and previous(maps, 0, A_BLOCK)[1] < A_BLOCK
        # the edge frame in front of buffer 256 of the second: a zero lead-in finds it at j = 325, the real one does not
        edges = [(k, b, f) for k, b, _, f in planted["edge"] if b >= A_BLOCK]
        assert (1, A_BLOCK) in [(k, b) for k, b, _ in edges]
        for k, b, f in edges:
            assert (b, LEAD - 1) in [(c, j) for c, j, _ in S.found(withouts[k], f)] and not S.found(wants[k], f), (k, b)
    return maps, wants, own, planted


# ------------------------------------------------------------------------------------------------- leg B
B_RECEIVERS = 16384
B_USED = (0, 1, 255, 256, 257, 4095, 4096, 16382, 16383)
B_TWICE = (0, 256, 4096, 16383)
B_UNUSED = (2, 254, 258, 16381)


class _Lazy(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, key):
        value = self[key] = self.make()
        return value


class WideModel(S.SeamModel):
    """SeamModel for any number of receivers: a receiver's stream and carry are made when it is first used.  alias: receiver
    r uses the stream and the carry of r & alias -- what an implementation that truncates the receiver index computes."""

    def __init__(self, carry: bool = True, alias: Optional[int] = None):   # (not SeamModel's: it makes every stream at once)
        self.mode, self.carry_on, self.alias = 0, carry, alias
        self.streams = _Lazy(self._new)
        self.carry = _Lazy(lambda: np.zeros((LEAD, 2), dtype=np.int16))

    def feed(self, iq, receivers):
        m = np.asarray(receivers, dtype=np.int64)
        return super().feed(iq, m if self.alias is None else m & self.alias)


def _after(m: np.ndarray, r: int, behind: int) -> Optional[int]:
    hits = [b for b in range(behind + 1, len(m)) if int(m[b]) == r]
    return hits[0] if hits else None


def _chain(m: np.ndarray, receivers: Sequence[int]) -> Optional[List[int]]:
    """buffers b0 < b1 < ... with m[b_i] == receivers[i], each the first one behind the one before"""
    out, at = [], -1
    for r in receivers:
        at = _after(m, r, at)
        if at is None:
            return None
        out.append(at)
    return out


@lru_cache(maxsize=None)
def leg_b_maps():
    """Four maps of 20 buffers over B_USED: every member in every pass, B_TWICE twice at least; in the first pass receiver
    0, then 256, then 4096, then 0 again; in the second 16383 twice.  -> (maps, those four buffers, those two)"""
    rng = np.random.default_rng([0x5EA3, 0xB])
    must = list(B_USED) + list(B_TWICE)
    maps, chains = [], []
    for k in range(4):
        while True:
            m = np.array(must + [int(x) for x in rng.choice(B_USED, size=N - len(must))], dtype=np.uint32)
            rng.shuffle(m)
            chain = _chain(m, (0, 256, 4096, 0)) if k == 0 else _chain(m, (16383, 16383)) if k == 1 else []
            if chain is not None:
                break
        maps.append(m)
        chains.append(chain)
    return maps, chains[0], chains[1]


@lru_cache(maxsize=None)
def leg_b_inputs():
    """The dense capture four times, seam frames in rotation, and the aircraft X: receiver 0 hears its DF17 early in the
    first pass; replies to it follow in a buffer of receiver 256, in one of 4096 (neither has heard X: not emitted) and in
    a later one of receiver 0 (1000); in the second pass receiver 16383 hears the DF17 and, a buffer later, the reply."""
    maps, (b_learn, b_256, b_4096, b_reply), (b_learn2, b_reply2) = leg_b_maps()
    inputs = [SS.dense().copy() for _ in maps]
    planted = plant_seams(inputs, maps)
    teach(inputs[0], b_learn, DF17_X, 0)
    teach(inputs[0], b_256, REPLY_X, 1)
    teach(inputs[0], b_4096, REPLY_X, 2)
    teach(inputs[0], b_reply, REPLY_X, 3)
    teach(inputs[1], b_learn2, DF17_X, 4)
    teach(inputs[1], b_reply2, REPLY_X, 5)
    for x in inputs:
        x.setflags(write=False)
    return inputs, maps, planted


@lru_cache(maxsize=None)
def leg_b_case(mode: str):
    """mode "both": carry and a filter per receiver; "scoring": a filter per receiver, no carry.  -> (the model's lists, the model)"""
    carry = mode == "both"
    inputs, maps, planted = leg_b_inputs()
    (b_learn, b_256, b_4096, b_reply), (b_learn2, b_reply2) = leg_b_maps()[1:]
    for m in maps:
        count = {r: int((m == r).sum()) for r in B_USED}
        assert set(int(x) for x in m) == set(B_USED) and all(count[r] >= 2 for r in B_TWICE), count
    own = WideModel(carry)
    wants = feed_all(own, inputs, maps)
    assert_dense(wants, maps)
    # X: learnt by receiver 0, its reply not emitted for 256 and 4096, emitted for 0; then the same for 16383 alone
    assert [b for b, _, _ in emissions(wants[0], DF17_X)] == [b_learn] and emissions(wants[0], REPLY_X) == [(b_reply, False, 1000)]
    assert [b for b, _, _ in emissions(wants[1], DF17_X)] == [b_learn2] and emissions(wants[1], REPLY_X) == [(b_reply2, False, 1000)]
    # a receiver index cut to 8 or to 12 bits gives another list: 256 and 4096 then share receiver 0's filter and carry
    for alias, b_heard in ((0xFF, b_256), (0xFFF, b_4096)):
        cut = feed_all(WideModel(carry, alias), inputs, maps)
        assert sum(cut, []) != sum(wants, [])
        assert (b_heard, False, 1000) in emissions(cut[0], REPLY_X), (alias, emissions(cut[0], REPLY_X))
    if carry:
        withouts = feed_all(WideModel(False), inputs, maps)
        found = assert_seams_found(wants, withouts, planted, missing=2)
        shareds = feed_all(SS.SharedFilterModel(B_RECEIVERS), inputs, maps)
        SS.assert_input_is_for_this(B_RECEIVERS, list(zip(inputs, maps)), wants, withouts, shareds, [f for _, _, f in found])
        # the receivers that occur twice have a seam inside a pass, and some planted frame is found at one
        inside_a_pass = [(k, b) for k, b, _ in found if previous(maps, k, b)[0] == k and int(maps[k][b]) in B_TWICE]
        assert inside_a_pass
    else:
        shareds = feed_all(WideModel(False, alias=0), inputs, maps)   # (every receiver the same stream: one shared filter)
        RS.assert_tells_apart(B_RECEIVERS, sum(wants, []), sum(shareds, []))
    for r in B_UNUSED:
        assert not any(own.table(r))
    return wants, own


# ------------------------------------------------------------------------------------------------- leg C
C_RECEIVERS = 3
C_MAP0 = np.array([0, 1, 2] * 6 + [1, 2], dtype=np.uint32)
C_MAP1 = np.array([0, 1, 2, 0, 1, 0, 1, 2, 0, 1, 2, 0, 1, 2, 1, 2, 0, 1, 2, 0], dtype=np.uint32)
C_SILENT = (0, 5, 6, 7, 18, 19)
DF11_C0, DF11_C7 = synth.df11_frame(0x4C0001), synth.df11_frame(0x4C0007)


@lru_cache(maxsize=None)
def leg_c_gaps_case():
    """A dense pass, then the pass with the gaps: buffer 0 silent (a leading gap; its seam frame lies at the end of receiver
    0's last buffer of the pass before), buffers 5, 6, 7 silent with seam frames in front of 5 (a reply to X, which receiver
    0 learnt in buffer 3) and 7 (a DF11) and nothing in front of 6, buffers 18 and 19 silent with a reply to X in front of 19
    (the fill behind the last hit).  Every frame in front of a silent buffer lies wholly inside the last 326 samples of the
    buffer before it; the straddling ones are kept for dense buffers.  -> (inputs, maps, the model's lists, the model)"""
    maps = [C_MAP0, C_MAP1]
    inputs = [SS.dense().copy(), SS.dense().copy()]
    planted = plant_seams(inputs[:1], maps[:1], every=2)
    silence(inputs[1], C_SILENT)
    teach(inputs[1], 3, DF17_X)
    gaps = {0: DF11_C0, 5: REPLY_X, 7: DF11_C7, 19: REPLY_X2}
    for n, (b, f) in enumerate(gaps.items()):
        assert int(C_MAP1[b]) == (2 if b == 7 else 0)
        plant_at(inputs, maps, 1, b, -190, f, n)
    n = 100
    for b, kind in ((1, "straddle"), (4, "straddle"), (11, "straddle"), (13, "last"), (14, "edge"), (17, "straddle")):
        pk, pb = previous(maps, 1, b)
        assert b not in C_SILENT and (pk == 0 or pb not in C_SILENT)
        planted[kind].append((1, b, int(C_MAP1[b]), plant_kind(inputs[pk], pb, inputs[1], b, kind, n)))
        n += 1
    assert all(is_silent(inputs[1], b) for b in C_SILENT)
    assert previous(maps, 1, 0)[0] == 0                                 # buffer 0's lead-in comes from the pass before
    own, without = S.SeamModel(C_RECEIVERS), S.SeamModel(C_RECEIVERS, carry=False)
    wants, withouts = feed_all(own, inputs, maps), feed_all(without, inputs, maps)
    assert_seams_found(wants, withouts, planted)
    assert_dense(wants, maps)
    for b in C_SILENT:
        assert not in_buffer(withouts[1], b), b
        got = in_buffer(wants[1], b)
        if b in gaps:   # exactly the planted frame, across the seam
            assert got and {k[4] for k in got} == {gaps[b]} and all(k[1] < LEAD for k in got), (b, got)
        else:
            assert not got, (b, got)
    assert emissions(wants[1], REPLY_X) == [(5, True, 1000)] and emissions(wants[1], REPLY_X2) == [(19, True, 1000)]
    return inputs, maps, wants, own


C_WARM = 3   # dense passes in front: with the priming pass they go through all four slots once


@lru_cache(maxsize=None)
def leg_c_only_seams_case():
    """Three dense passes, a dense pass K that ends every receiver's stream with a frame wholly inside its last 326 samples
    (receiver 0: a reply to X, learnt in K), and a pass of 20 silent buffers: no own hit at all, three seam records' worth
    of messages.  The dense passes in front take every slot through a pass with hits first, so that the silent pass finds
    the work arrays of its slot as such a pass leaves them.  -> (inputs, maps, the model's lists, the model, frames of the
    silent pass by buffer)"""
    rng = np.random.default_rng([0x5EA3, 0xC])
    maps = [rng.integers(0, C_RECEIVERS, size=N).astype(np.uint32) for _ in range(C_WARM + 1)]
    maps.append(np.array([0, 1, 2] * 6 + [0, 1], dtype=np.uint32))
    k_last, k_silent = C_WARM, C_WARM + 1
    assert set(int(x) for x in maps[k_last]) == {0, 1, 2}
    inputs = [SS.dense().copy() for _ in maps]
    planted = plant_seams(inputs[:k_silent], maps[:k_silent])
    silence(inputs[k_silent], range(N))
    b_learn = [b for b in range(N) if int(maps[k_last][b]) == 0][0]
    teach(inputs[k_last], b_learn, DF17_X)
    ends = {0: REPLY_X, 1: DF11_C0, 2: DF11_C7}     # (buffer r of the silent pass is receiver r's first)
    for n, (b, f) in enumerate(ends.items()):
        assert previous(maps, k_silent, b)[0] == k_last
        plant_at(inputs, maps, k_silent, b, -190, f, n)
    assert not inputs[k_silent].any()
    own, without = S.SeamModel(C_RECEIVERS), S.SeamModel(C_RECEIVERS, carry=False)
    wants, withouts = feed_all(own, inputs, maps), feed_all(without, inputs, maps)
    assert_seams_found(wants, withouts, planted, missing=2)
    assert_dense(wants, maps, range(k_silent))
    assert not withouts[k_silent]
    assert [(k[0], k[4]) for k in wants[k_silent]] == sorted(ends.items()) and all(k[1] < LEAD for k in wants[k_silent])
    assert wants[k_silent][0][3] == 1000
    return inputs, maps, wants, own, ends


# ------------------------------------------------------------------------------------------------- leg D
D_RECEIVERS, D_FIRST_SEAM = 3, 8
DF17_D = synth.df17_frame(0x4D0001, 0x2233445566778)


@lru_cache(maxsize=None)
def leg_d_case():
    """A dense pass, then the judged one: its buffer 0 starts with a DF17 whose first preamble pulse is sample 0, behind a
    full-scale last sample of its receiver's previous buffer (in the pass before) -- the pass's own scan finds it at j = 325
    against zeros and that hit is dropped, the real lead-in does not find it: D(0) = 1, S(0) = 0.  No seam frame before
    buffer 8, ordinary ones from there on.  -> (inputs, maps, the model's lists, the model)"""
    rng = np.random.default_rng([0x5EA3, 0xD])
    maps = [rng.integers(0, D_RECEIVERS, size=N).astype(np.uint32) for _ in range(2)]
    inputs = [SS.dense().copy(), SS.dense().copy()]
    planted = plant_seams(inputs, maps, every=2, skip=lambda k, b: k == 1 and b < D_FIRST_SEAM)
    assert previous(maps, 1, 0)[0] == 0
    plant_at(inputs, maps, 1, 0, 0, DF17_D, loud=True)
    own, without = S.SeamModel(D_RECEIVERS), S.SeamModel(D_RECEIVERS, carry=False)
    wants, withouts = feed_all(own, inputs, maps), feed_all(without, inputs, maps)
    assert_seams_found(wants, withouts, planted, missing=1)
    assert_dense(wants, maps)
    assert [(b, j) for b, j, _ in S.found(withouts[1], DF17_D)] == [(0, LEAD - 1)]
    assert not S.found(sum(wants, []), DF17_D)
    at_seams = [k[0] for k in wants[1] if k[1] < LEAD]
    assert at_seams and min(at_seams) >= D_FIRST_SEAM, at_seams[:4]
    assert [b for k, b, f in seam_frames(planted) if k == 1 and b >= D_FIRST_SEAM and found_at_the_seam(wants, k, b, f)]
    return inputs, maps, wants, own
