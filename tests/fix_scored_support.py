"""Shared by the tests of device-side scoring under error correction (tests/test_fix_scored_cpu.py,
tests/test_gpu_fix_scored.py): a dense stream in which the ORDER of damaged and clean frames inside one pass decides
what is repaired, its classes, and the conditions the CPU restatement must meet on it so that a GPU comparison with the
restatement cannot pass vacuously."""
import numpy as np

from dump1090_rs_amd import synth
from tests import fix2_support as f2
from tests import fix_support as fs

CHUNK = fs.CHUNK
N_BUFFERS = 20                      # > 16: such a pass is ordered and scored on the device once the stream is known dense
LATE, EARLY, ONLY18 = 0x4840D6, 0x3C6589, 0x71BE05
ME = 0x58C382D690C8AC
ADDRESS_BITS = list(range(8, 32))   # message bits of the address field


def df18_frame(icao: int, me: int) -> bytes:
    """A valid 112-bit DF18 (CF 0): what a non-transponder device sends; adds icao | 1 << 25 to the filter."""
    body = bytes([0x90]) + icao.to_bytes(3, "big") + (me & ((1 << 56) - 1)).to_bytes(7, "big")
    return body + synth.crc24(body).to_bytes(3, "big")


def order_stream(seed: int = 9100):
    """(iq, {slot: (class, clean frame)}) -- slots as in fix2_support.pair_stream (slot_of maps a message key to one).
    LATE is heard cleanly first (slot 0) and every damaged copy of its DF17 and DF18 frames follows; EARLY's damaged
    copies come first and its first clean frame only in buffer 2, with more copies behind it; ONLY18 is only ever heard
    as DF18, which adds addr | 1 << 25 and so never makes its plain address known.  Classes:
      late1 / late2        one / two flipped bits of LATE's DF17, none in the address field, none at bit 111
      addr1 / addr2        ... with a flipped bit inside the address field, bits 8..31 (every one of them)
      last1                bit 111
      df18_1 / df18_2      LATE's DF18 frame damaged (its address is known from the DF17)
      early1 / early2      EARLY's DF17 damaged, before its first clean frame
      after1 / after2      ... behind it
      only18               ONLY18's DF18 damaged: never repaired
      clean, weak          clean frames; `weak` ones at low amplitude, where the trial phases of one position disagree"""
    late, early = synth.df17_frame(LATE, ME), synth.df17_frame(EARLY, ME + 0x1000)
    late18, only18 = df18_frame(LATE, ME + 0x2000), df18_frame(ONLY18, ME + 0x3000)
    plain = [b for b in range(32, 111)]
    frames = [("clean", late, late), ("clean", only18, only18), ("clean", only18, only18)]
    frames += [("early1", fs.flip(early, b), early) for b in (ADDRESS_BITS + plain)[::3] + [111]]
    frames += [("early2", f2.flip2(early, a, a + 17 + k % 40), early) for k, a in enumerate(range(6, 60, 2))]
    frames += [("late1", fs.flip(late, b), late) for b in plain[::2]]
    frames += [("late2", f2.flip2(late, a, a + 3 + k % 29), late) for k, a in enumerate(range(32, 80))]
    frames += [("addr1", fs.flip(late, b), late) for b in ADDRESS_BITS]
    frames += [("addr2", f2.flip2(late, a, b), late) for a in ADDRESS_BITS for b in (a + 1 if a < 31 else 40, 55 + a)]
    frames += [("last1", fs.flip(late, 111), late)] * 24
    frames += [("df18_1", fs.flip(late18, b), late18) for b in (ADDRESS_BITS + plain)[::3] + [111]]
    frames += [("df18_2", f2.flip2(late18, a, a + 9 + k % 50), late18) for k, a in enumerate(range(5, 60, 2))]
    frames += [("only18", fs.flip(only18, b), only18) for b in range(20, 100, 8)]
    frames += [("only18", f2.flip2(only18, b, b + 5), only18) for b in range(20, 100, 8)]
    assert len(frames) <= 2 * f2.PER_BUFFER - 1, len(frames)
    frames += [("weak", late, late)] * (2 * f2.PER_BUFFER - len(frames))
    frames += [("clean", early, early)]                                     # buffer 2, slot 0
    frames += [("after1", fs.flip(early, b), early) for b in (ADDRESS_BITS + plain)[1::3] + [111]]
    frames += [("after2", f2.flip2(early, a, a + 11 + k % 45), early) for k, a in enumerate(range(7, 61, 2))]
    n_slots = N_BUFFERS * f2.PER_BUFFER
    weak = [late, early, late18]
    frames += [("weak", weak[k % 3], weak[k % 3]) for k in range(n_slots - len(frames))]
    iq = np.concatenate([synth.noise_numpy(CHUNK, seed + k) for k in range(N_BUFFERS)])
    bursts, want = [], {}
    for slot, (kind, frame, good) in enumerate(frames):
        t = (slot // f2.PER_BUFFER) * CHUNK + f2.FIRST + f2.SPACING * (slot % f2.PER_BUFFER)
        amplitude = 2600 + 37 * (slot % 120) if kind == "weak" else 21000 + 97 * (slot % 50)
        bursts.append(synth.Burst(5 * t + (slot % 5), amplitude, slot % 16, frame))
        want[slot] = (kind, good)
    synth.add_bursts(iq, bursts)
    return iq, want


def damaged_addresses() -> list:
    """the addresses one flipped address bit turns LATE and EARLY into (order_stream's addr1 / addr2 / early1 copies
    carry them): never heard there"""
    return [LATE ^ (1 << (31 - b)) for b in ADDRESS_BITS] + [EARLY ^ (1 << (31 - b)) for b in ADDRESS_BITS]


def victim_stream(seed: int, victims: list, n_buffers: int = N_BUFFERS):
    """(iq, {slot: (class, clean frame)}), slots as above: for each address of `victims` a one-bit and a two-bit copy of
    its DF17 BEFORE its first clean frame (`before`), that frame (`first`), and a one-bit and a two-bit copy behind it
    (`after1`, `after2`); the rest weak clean frames of LATE, for density.  Behind order_stream in one capture, with
    damaged_addresses() as victims: an address exchange that took a repairable DF17's damaged address for one the capture
    adds would score `first` as known and repair `before`."""
    frames = []
    for k, v in enumerate(victims):
        good = synth.df17_frame(v, ME + 0x5000 + k)
        frames += [("before", fs.flip(good, 40 + k % 60), good), ("before", f2.flip2(good, 33 + k % 50, 90 + k % 20), good),
                   ("first", good, good), ("after1", fs.flip(good, 45 + k % 60), good),
                   ("after2", f2.flip2(good, 35 + k % 50, 88 + k % 20), good)]
    n_slots = n_buffers * f2.PER_BUFFER
    assert len(frames) <= n_slots
    # spread over the buffers: every buffer holds victims and filler
    late = synth.df17_frame(LATE, ME)
    per = (len(frames) + n_buffers - 1) // n_buffers
    per += -per % 5                                     # (an address's five frames stay in one buffer, in order)
    slots = {}
    for i, f in enumerate(frames):
        slots[(i // per) * f2.PER_BUFFER + i % per] = f
    iq = np.concatenate([synth.noise_numpy(CHUNK, seed + k) for k in range(n_buffers)])
    bursts, want = [], {}
    for slot in range(n_slots):
        kind, frame, good = slots.get(slot, ("weak", late, late))
        t = (slot // f2.PER_BUFFER) * CHUNK + f2.FIRST + f2.SPACING * (slot % f2.PER_BUFFER)
        amplitude = 2600 + 37 * (slot % 120) if kind == "weak" else 21000 + 97 * (slot % 50)
        bursts.append(synth.Burst(5 * t + (slot % 5), amplitude, slot % 16, frame))
        want[slot] = (kind, good)
    synth.add_bursts(iq, bursts)
    return iq, want


def check_victims(keys: list, want: dict, first_buffer: int, mode: int = 3) -> None:
    """A capture on an empty filter whose buffers from `first_buffer` on are a victim_stream: no copy in front of an
    address's first clean frame yields a message (the address is not known before), that frame scores 1400 -- or 1800 where
    two trial phases of its position slice it clean: the first adds the address, the second finds it --, and the copies
    behind it come back (mode 1: the one-bit ones)."""
    got = {}
    for k in keys:
        if k[4] >= first_buffer:
            kk = (k[0], k[1], k[2], k[3], k[4] - first_buffer, k[5])
            got.setdefault(f2.slot_of(kk), []).append((k[0], k[1]))
    count = {}
    for slot, (kind, good) in want.items():
        msgs = got.get(slot, [])
        if kind == "before":
            assert msgs == [], (slot, kind, msgs)
        elif kind == "first":
            assert msgs and all(m[0] == good and m[1] in CLEAN for m in msgs), (slot, kind, msgs)
        elif kind == "after1" or (kind == "after2" and mode == 3):
            assert msgs and all(m[0] == good for m in msgs), (slot, kind, msgs)
            count[kind] = count.get(kind, 0) + all(m[1] == (1200 if kind == "after1" else 1100) for m in msgs)
        else:
            continue
        count[kind + "_n"] = count.get(kind + "_n", 0) + 1
    assert count["before_n"] >= 40 and count["first_n"] >= 20 and count["after1"] >= 20, count
    assert mode != 3 or count["after2"] >= 20, count


CLEAN = (1800, 1400)   # where a neighbouring trial phase slices the damaged bits right, the clean frame wins the position
ONE_BIT = ("late1", "addr1", "last1", "df18_1")
TWO_BIT = ("late2", "addr2", "df18_2")


def by_slot(keys: list) -> dict:
    """{slot: [(bytes, score), ...]} of every message of a call"""
    out = {}
    for k in keys:
        out.setdefault(f2.slot_of(k), []).append((k[0], k[1]))
    return out


def check_first_call(keys: list, want: dict) -> None:
    """A call on an empty filter: no early copy and no ONLY18 copy yields a message; every late one-bit copy comes back at
    1200 and every late two-bit copy at 1100 with the clean bytes (or higher, where another trial phase sliced a damaged
    bit right: best of five); at least 20 of each class at its own score."""
    got = by_slot(keys)
    count = {}
    for slot, (kind, good) in want.items():
        msgs = got.get(slot, [])
        if kind in ("early1", "early2", "only18"):
            assert msgs == [], (slot, kind, msgs)
        elif kind in ONE_BIT + ("after1",):
            assert msgs and all(m[0] == good and m[1] in (1200,) + CLEAN for m in msgs), (slot, kind, msgs)
            count[kind] = count.get(kind, 0) + all(m[1] == 1200 for m in msgs)
        elif kind in TWO_BIT + ("after2",):
            assert msgs and all(m[0] == good and m[1] in (1100, 1200) + CLEAN for m in msgs), (slot, kind, msgs)
            count[kind] = count.get(kind, 0) + all(m[1] == 1100 for m in msgs)
    for kind in ONE_BIT + TWO_BIT + ("after1", "after2"):
        assert count.get(kind, 0) >= 20, (kind, count)
    assert sum(kind == "early1" for kind, _ in want.values()) >= 20 and sum(kind == "early2" for kind, _ in want.values()) >= 20


def check_second_call(keys: list, want: dict) -> None:
    """... and the same stream again without a flush: the early copies come back too; ONLY18's still do not."""
    got = by_slot(keys)
    count = {}
    for slot, (kind, good) in want.items():
        msgs = got.get(slot, [])
        if kind == "only18":
            assert msgs == [], (slot, kind, msgs)
        elif kind == "early1":
            assert msgs and all(m[0] == good and m[1] in (1200,) + CLEAN for m in msgs), (slot, kind, msgs)
            count[kind] = count.get(kind, 0) + all(m[1] == 1200 for m in msgs)
        elif kind == "early2":
            assert msgs and all(m[0] == good and m[1] in (1100, 1200) + CLEAN for m in msgs), (slot, kind, msgs)
            count[kind] = count.get(kind, 0) + all(m[1] == 1100 for m in msgs)
    assert count.get("early1", 0) >= 20 and count.get("early2", 0) >= 20, count


def competing_positions(iq, keys: list) -> list:
    """Message keys at positions where the five trial phases compete: one phase slices a DF17/18 clean (residual 0),
    another slices it with exactly one wrong bit in 5..111.  From the oracle's trials and CRC alone."""
    from oracle import binding
    single = set()
    for b in range(5, 112):
        e = bytearray(14)
        e[b >> 3] = 0x80 >> (b & 7)
        single.add(synth.crc24(bytes(e[:11])) ^ int.from_bytes(e[11:], "big"))
    wanted = {}
    for k in keys:
        wanted.setdefault(k[4], {})[k[2]] = k
    out = []
    for chunk, at in sorted(wanted.items()):
        _, trials = binding.all_trials(iq[chunk * CHUNK:(chunk + 1) * CHUNK], chunk)
        per_j = {}
        for t in trials:
            j = int(t["j_tp"]) & 0xFFFFFF
            if j not in at:
                continue
            m = bytes(t["msg"])
            if m[0] >> 3 not in (17, 18):
                continue
            per_j.setdefault(j, []).append(synth.crc24(m[:11]) ^ int.from_bytes(m[11:], "big"))
        for j, res in per_j.items():
            if 0 in res and any(r in single for r in res):
                out.append(at[j])
    return out
