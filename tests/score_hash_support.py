"""Shared by the tests of the first-adder table of device-side scoring (tests/test_score_hash_cpu.py,
tests/test_gpu_score_hash.py): the table's size rule and home-slot formula restated (csrc/adsb_device.h: score_hash_size,
score_hash_slot), addresses chosen by home slot, and dense streams whose adders form ONE cluster that wraps from the
last slot of the table to slot 0, with addresses that are looked up across it and must not be found."""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from dump1090_rs_amd import synth
from tests import formats_support as F

CHUNK = F.CHUNK
N_BUFFERS = 17                       # > 16: such a pass is ordered and scored on the device once the stream is known dense
MUL = 2654435761
AP_DFS = (0, 4, 5, 16, 20, 21) + tuple(range(24, 32))

# home slot relative to the table size S (taken mod S) -> how many addresses
SMALL = {"taught": {-2: 30, -1: 60, 0: 30, 1: 10}, "strangers": {-1: 20, 0: 10, -3: 10, 2: 5}}
LARGE = {"taught": {k: 100 for k in (-3, -2, -1, 0, 1, 2)}, "strangers": {-1: 40, 0: 16, -4: 20}}
FORMS = {"small": SMALL, "large": LARGE}


# ------------------------------------------------------------------------------------ the two formulas, restated
def hash_size(max_chunks: int) -> int:
    """Slots of ScoreDev::hash in a context created for `max_chunks` buffers: the smallest power of two >= 2 x the hits
    a pass may have to be scored on the device, min(4096 + 1024 max_chunks, 262144)."""
    cap = min(4096 + 1024 * max_chunks, 262144)
    size = 1
    while size < 2 * cap:
        size <<= 1
    return size


def home(v: int, max_chunks: int) -> int:
    """The slot the probes of value v start at."""
    return (((v * MUL) & 0xFFFFFFFF) >> 8) & (hash_size(max_chunks) - 1)


_h24: Optional[np.ndarray] = None


def _homes24() -> np.ndarray:
    """(v * MUL mod 2^32) >> 8 of every 24-bit value, one numpy pass"""
    global _h24
    if _h24 is None:
        v = np.arange(1 << 24, dtype=np.uint64)
        _h24 = (((v * np.uint64(MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)).astype(np.uint32)
    return _h24


def addresses_at(home_slot: int, max_chunks: int) -> np.ndarray:
    """Every 24-bit value whose home is `home_slot` (taken mod the table size), ascending."""
    size = hash_size(max_chunks)
    return np.nonzero((_homes24() & np.uint32(size - 1)) == np.uint32(home_slot % size))[0].astype(np.uint32)


def supply(max_chunks: int) -> int:
    """The fewest addresses any home slot has."""
    size = hash_size(max_chunks)
    return int(np.bincount(_homes24() & np.uint32(size - 1), minlength=size).min())


# ------------------------------------------------------------------------------------ addresses by home slot
class Picker:
    """Distinct addresses >= 0x100000 by home slot, fixed seed."""

    def __init__(self, max_chunks: int, seed: int):
        self.max_chunks = max_chunks
        self.size = hash_size(max_chunks)
        self.r = np.random.default_rng([0x5C0E, seed])
        self.used: set = set()

    def at(self, rel_slot: int, count: int) -> List[int]:
        cands = [int(a) for a in addresses_at(rel_slot, self.max_chunks) if a >= 0x100000 and int(a) not in self.used]
        assert len(cands) >= count, (rel_slot, len(cands), count)
        out = [cands[i] for i in self.r.permutation(len(cands))[:count]]
        assert all(home(a, self.max_chunks) == rel_slot % self.size for a in out)
        self.used.update(out)
        return out

    def cluster(self, plan: Dict[int, int]) -> List[int]:
        return [a for rel, n in plan.items() for a in self.at(rel, n)]

    def elsewhere(self, count: int) -> List[int]:
        """ordinary aircraft: homes at least 4096 slots from the cluster on either side"""
        out = []
        while len(out) < count:
            a = 0x100000 + int(self.r.integers(0, 0xE00000))
            if a not in self.used and 4096 <= home(a, self.max_chunks) < self.size - 4096:
                self.used.add(a)
                out.append(a)
        return out


# ------------------------------------------------------------------------------------ streams
def place(frames: Sequence[bytes], n_buffers: int, noise_seed: int, per_buffer: Optional[int] = None) -> np.ndarray:
    """`frames` spread evenly over `n_buffers` buffers of noise, in order: frame q in buffer q // per_buffer, one per
    (131072 - 400) // per_buffer samples from sample 200, tick offset q % 5, amplitude AMPLITUDES[q % 5]."""
    per_buffer = per_buffer or -(-len(frames) // n_buffers)
    assert len(frames) <= per_buffer * n_buffers
    gap = (CHUNK - 400) // per_buffer
    assert gap >= F.SPAN + 40, gap
    iq = synth.noise_numpy(n_buffers * CHUNK, seed=noise_seed)
    synth.add_bursts(iq, [synth.Burst(5 * ((q // per_buffer) * CHUNK + 200 + (q % per_buffer) * gap) + q % 5, F.AMPLITUDES[q % 5],
                                      q % 16, f) for q, f in enumerate(frames)])
    return iq


class _Frames:
    def __init__(self, seed: int):
        self.r = np.random.default_rng([0xF4A3, seed])

    def u(self, bits: int) -> int:
        return int.from_bytes(self.r.bytes((bits + 7) // 8), "big") >> (-bits % 8)

    def df17(self, a: int) -> bytes:
        return F.es_frame(17, a, self.u(56))

    def df18(self, a: int) -> bytes:
        return F.es_frame(18, a, self.u(56))

    def df11(self, a: int) -> bytes:
        return F.df11_frame(a, 0)

    def reply(self, a: int, dfs: Sequence[int]) -> bytes:
        return F.ap_frame(dfs[int(self.r.integers(0, len(dfs)))], a, self.u(64))

    def shuffled(self, frames: list) -> list:
        return [frames[i] for i in self.r.permutation(len(frames))]


@dataclass
class Colliding:
    max_chunks: int
    form: str
    iq: np.ndarray
    taught: List[int]
    strangers: List[int]
    per_buffer: int
    teachers: Dict[int, List[int]] = field(default_factory=dict)   # address -> frame indices of its DF17 / DF11 (IID 0)
    extra_taught: List[List[int]] = field(default_factory=list)    # (multi_capture: the later shards' clusters)
    damaged: Dict[bytes, Tuple[int, bool]] = field(default_factory=dict)   # (fix=True: clean frame -> (address, taught))

    def at_home(self, rel_slot: int) -> List[int]:
        size = hash_size(self.max_chunks)
        return [a for a in self.taught if home(a, self.max_chunks) == rel_slot % size]


def _colliding_frames(fr: _Frames, taught: List[int], strangers: List[int]) -> Tuple[list, Dict[int, List[int]]]:
    """The frame order of the colliding stream: (kind, address, frame) in transmission order."""
    half = set(fr.shuffled(list(taught))[: len(taught) // 2])
    before = [("reply_before", a, fr.reply(a, (4,))) for a in taught if a in half]
    teach = fr.shuffled([("teach", a, fr.df17(a)) for a in taught] +
                        [("stranger_reply", a, fr.reply(a, (4, 20))) for a in strangers])
    again = set(fr.shuffled(list(taught))[: len(taught) // 2])
    after = fr.shuffled([("reply", a, fr.reply(a, (4, 5, 20, 21))) for a in taught] +
                        [("teach_again", a, fr.df17(a)) for a in taught if a in again] +
                        [("teach_again", a, fr.df11(a)) for a in taught if a not in again] +
                        [("stranger_df18", a, fr.df18(a)) for a in strangers] +
                        [("stranger_reply", a, fr.reply(a, (5,))) for a in strangers])
    frames = before + teach + after
    teachers: Dict[int, List[int]] = {}
    for q, (kind, a, _) in enumerate(frames):
        if kind.startswith("teach"):
            teachers.setdefault(a, []).append(q)
    return frames, teachers


_streams: dict = {}


def colliding_stream(max_chunks: int, form: str = "small", seed: int = 1, fix: bool = False) -> Colliding:
    """17 buffers for a context created for `max_chunks` buffers.  With S its table size: the taught addresses of the form
    (SMALL: 130 keys at homes S-2, S-1, 0, 1 -- one cluster that wraps past the last slot; LARGE: 600 at S-3 .. 2) and
    strangers, never taught, at homes inside the cluster, at its wrap and in front of it.  In order: a DF4 reply to half
    of the taught addresses before anything teaches them; a shuffled block of one DF17 per taught address and DF4/DF20
    replies to strangers; a shuffled block of a DF4/5/20/21 reply to every taught address, a second DF17 of half of them, a
    DF11 (IID 0) of the other half, a DF18 of every stranger (adds addr | 1 << 25: no lookup may find it) and a DF5 reply
    to every stranger.  `fix`: behind all that a DF17 with message bit 40 flipped of ten taught addresses and of ten
    strangers (repairable under ADSB_FIX_1BIT where the address is in the filter)."""
    key = (hash_size(max_chunks), form, seed, fix)
    if key not in _streams:
        pk = Picker(max_chunks, seed)
        taught, strangers = pk.cluster(FORMS[form]["taught"]), pk.cluster(FORMS[form]["strangers"])
        assert min(taught + strangers) >= 0x100000 and len(set(taught + strangers)) == len(taught) + len(strangers)
        fr = _Frames(seed)
        frames, teachers = _colliding_frames(fr, taught, strangers)
        damaged = {}
        if fix:
            for a, known in [(a, True) for a in taught[::13][:10]] + [(a, False) for a in strangers[::4][:10]]:
                good = fr.df17(a)
                damaged[good] = (a, known)
                frames.append(("damaged", a, F.flip(good, 40)))
            assert len(damaged) == 20
        per_buffer = -(-len(frames) // N_BUFFERS)
        iq = place([f for _, _, f in frames], N_BUFFERS, 0x5C00 + seed, per_buffer)
        _streams[key] = Colliding(max_chunks, form, iq, taught, strangers, per_buffer, teachers, damaged=damaged)
    return _streams[key]


def teaching_stream(addresses: List[int], max_chunks: int, seed: int = 2) -> np.ndarray:
    """17 dense buffers that teach `addresses` (one DF17 each) among DF18s of ordinary aircraft heard twice (those add
    addr | 1 << 25: the filter's plain entries behind this pass are `addresses` and nothing else)."""
    key = ("teach", hash_size(max_chunks), tuple(addresses), seed)
    if key not in _streams:
        pk = Picker(max_chunks, 1000 + seed)
        pk.used.update(addresses)
        fr = _Frames(1000 + seed)
        n_fill = (20 * N_BUFFERS - len(addresses)) // 2
        frames = [fr.df17(a) for a in addresses] + [fr.df18(a) for a in pk.elsewhere(n_fill) for _ in range(2)]
        _streams[key] = place(fr.shuffled(frames), N_BUFFERS, 0x5D00 + seed)
    return _streams[key]


def replies_capture(groups: List[List[int]], avoid: Sequence[int] = (), seed: int = 3) -> np.ndarray:
    """17 buffers of ordinary dense fill (formats_support.fill_capture) per group of addresses; the last four hold, in
    this order: one DF17 of each of 22 addresses of ANOTHER cluster at the group's homes (contexts of 17 buffers; other
    addresses than the groups' and `avoid`) -- these occupy the home slots again, so that a lookup of a group's address
    walks on into whatever an earlier pass left behind them; for every address of the group a DF18; and, shuffled, a DF4
    reply, a DF20 reply and an all-call reply (DF11) with IID != 0 to it.  Nothing teaches the groups' addresses: the
    DF18 adds addr | 1 << 25 and scores 1400, and the reference emits none of the replies.  The DF18 and the DF11 are
    self-validating, so they reach the scoring kernels whatever the device's superset holds, and ask the filter about
    the plain address: a first-adder entry left behind by an earlier pass in the slot's table carries a small first
    index and scores the DF18 1800 and the DF11 1000.  (The DF4 / DF20 replies reach k_score only where the superset
    holds the address too.)"""
    key = ("replies", tuple(tuple(g) for g in groups), tuple(avoid), seed)
    if key not in _streams:
        pk = Picker(N_BUFFERS, 500 + seed)
        pk.used.update(a for g in groups for a in g)
        pk.used.update(avoid)
        other = pk.cluster({-2: 5, -1: 10, 0: 5, 1: 2})     # (the same for every group: each group is another table's)
        parts = []
        for k, g in enumerate(groups):
            fr = _Frames(2000 + seed + k)
            iq = F.fill_capture(0x5E00 + 16 * seed + k, N_BUFFERS)
            frames = fr.shuffled([fr.df17(a) for a in other]) + fr.shuffled([fr.df18(a) for a in g]) + \
                fr.shuffled([fr.reply(a, (4,)) for a in g] + [fr.reply(a, (20,)) for a in g] +
                            [F.df11_frame(a, 1 + (i + k) % 127) for i, a in enumerate(g)])
            iq[(N_BUFFERS - 4) * CHUNK:] = place(frames, 4, 0x5F00 + 16 * seed + k)
            parts.append(iq)
        _streams[key] = np.concatenate(parts)
    return _streams[key]


def multi_capture(n_shards: int, seed: int = 4) -> Colliding:
    """A capture of 17 n buffers for contexts of 17: the first 17 are the small form; every later run of 17 holds a
    DF4/5/20/21 reply to every address the runs before it taught (a device-scored shard finds those through
    ScoreDev::earlier), and a cluster of its own at the same homes: one DF17 per address, then a reply to each, a second
    DF17 of half of them, and DF5 replies to the first run's strangers."""
    key = ("multi", n_shards, seed)
    if key not in _streams:
        base = colliding_stream(N_BUFFERS, "small", seed)
        pk = Picker(N_BUFFERS, seed)
        pk.used.update(base.taught + base.strangers)
        pk.r = np.random.default_rng([0x5C0F, seed])
        parts, known, extra = [base.iq], list(base.taught), []
        for k in range(1, n_shards):
            fr = _Frames(3000 + seed + k)
            mine = pk.cluster(SMALL["taught"])
            frames = fr.shuffled([fr.reply(a, (4, 5, 20, 21)) for a in known] + [fr.df17(a) for a in mine])
            frames += fr.shuffled([fr.reply(a, (4, 5, 20, 21)) for a in mine] + [fr.df17(a) for a in mine[::2]] +
                                  [fr.reply(a, (5,)) for a in base.strangers])
            parts.append(place(frames, N_BUFFERS, 0x6000 + 16 * seed + k))
            known += mine
            extra.append(mine)
        _streams[key] = Colliding(N_BUFFERS, "small", np.concatenate(parts), base.taught, base.strangers, base.per_buffer,
                                  base.teachers, extra_taught=extra)
    return _streams[key]


# ------------------------------------------------------------------------------------ message keys and preconditions
def level_bits(x: float) -> bytes:
    return struct.pack("<d", float(x))


def key(m) -> tuple:
    """(chunk, j, try_phase, score, bytes, signal_level bits) of a library message (ModeSMessage)"""
    return (int(m.chunk), int(m.j), int(m.try_phase), int(m.score), m.buffer(), level_bits(m.signal_level))


def okey(w: dict) -> tuple:
    """... of an oracle message (oracle.binding.unpack)"""
    return (w["chunk"], w["j"], w["try_phase"], w["score"], w["buffer"], level_bits(w["signal_level"]))


def rkey(k: tuple) -> tuple:
    """... of a restatement key (fix_support.okey)"""
    return (k[4], k[2], k[3], k[1], k[0], level_bits(k[5]))


def ap_address(msg: bytes) -> Optional[int]:
    """The address an address/parity message answers for (its CRC residual), None for every other DF."""
    if msg[0] >> 3 not in AP_DFS:
        return None
    return synth.crc24(msg[:-3]) ^ int.from_bytes(msg[-3:], "big")


def replies_to(keys: List[tuple], addresses) -> List[tuple]:
    """the address/parity and all-call (DF11) messages of `keys` that answer for one of `addresses`"""
    who = set(addresses)
    return [k for k in keys if ap_address(k[4]) in who or (k[4][0] >> 3 == 11 and int.from_bytes(k[4][1:4], "big") in who)]


def known_replies(keys: List[tuple]) -> Dict[int, int]:
    """{address: address/parity messages at score 1000} of a list of keys"""
    out: Dict[int, int] = {}
    for k in keys:
        a = ap_address(k[4])
        if a is not None and k[3] == 1000:
            out[a] = out.get(a, 0) + 1
    return out


def check_preconditions(keys: List[tuple], s: Colliding, filter_table, taught: Optional[List[int]] = None) -> None:
    """On the oracle's list alone: every taught address has an address/parity message at 1000, no stranger has one, no
    such message belongs to anyone else, and the filter is far from the point where a context hands a pass back to the
    host (held + additions + 64 < 4096, csrc/adsb_collect.cpp)."""
    taught = list(s.taught if taught is None else taught)
    got = known_replies(keys)
    assert all(a in got for a in taught), [hex(a) for a in taught if a not in got][:8]
    assert not any(a in got for a in s.strangers), [hex(a) for a in s.strangers if a in got][:8]
    assert set(got) <= set(taught), [hex(a) for a in got if a not in set(taught)][:8]
    assert sum(v != 0 for v in filter_table) < 4096 - 64 - 600


def taught_twice(keys: List[tuple], s: Colliding) -> Tuple[List[int], List[int]]:
    """(taught addresses whose first teacher emission -- a DF17 or DF11 of theirs, nothing having answered for the
    address before it -- is followed IN ANOTHER BUFFER by one at 1800 / 1600; those of them whose first emission is at
    1400 / 750), both in list order."""
    first: Dict[int, Tuple[int, int]] = {}
    answered_early, twice = set(), []
    want = set(s.taught)
    for k in keys:
        a = ap_address(k[4])
        if a is not None:
            if a in want and a not in first and k[3] == 1000:
                answered_early.add(a)
            continue
        if k[4][0] >> 3 not in (11, 17):
            continue
        a = int.from_bytes(k[4][1:4], "big")
        if a not in want:
            continue
        if a not in first:
            assert k[3] in (1400, 750, 1800, 1600), k
            first[a] = (k[0], k[3])
        elif k[3] in (1800, 1600) and k[0] != first[a][0] and a not in twice and a not in answered_early:
            twice.append(a)
    return twice, [a for a in twice if first[a][1] in (1400, 750)]
