"""The part of the score-grid tests that needs no GPU: tests/score_rounds_support.py restates four fixed sizes of the
library and the arithmetic of its score grid, and tests/test_gpu_score_rounds.py composes its streams from that
restatement -- here it is held against the sources (a host program compiled from csrc/adsb_device.h and
csrc/adsb_scan_geometry.h; kHitCap and the cap expression as text), so that a changed constant fails here before a GPU leg
quietly tests nothing.  And the subset-sum helpers and the straddle finder on made-up counts."""
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import score_rounds_support as S
from tests.conftest import ROOT

CSRC = ROOT / "dump1090_rs_amd" / "csrc"
PROGRAM = r"""
#include <cstdio>
#include "adsb_device.h"
#include "adsb_scan_geometry.h"
int main()
{
    std::printf("%u %u %d %d %d %d\n", adsb::kTileBucket, adsb::kOrderBucket, adsb::kScoreBlocks, adsb::fastgeo::kTilesPerChunk,
                adsb::fastgeo::kTile, adsb::kChunkSamples);
    return 0;
}
"""


@pytest.fixture(scope="module")
def constants(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_rounds")
    src, exe = d / "score_rounds_host.cpp", d / "score_rounds_host"
    src.write_text(PROGRAM)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wextra",
                    "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)], check=True, cwd=d, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, check=True)
    return [int(x) for x in r.stdout.split()]


def test_the_restated_sizes_against_the_sources(constants):
    tile_bucket, order_bucket, score_blocks, tiles, tile, chunk = constants
    assert (tile_bucket, order_bucket, score_blocks, tiles, tile, chunk) == \
        (S.TILE_BUCKET, S.ORDER_BUCKET, S.SCORE_BLOCKS, S.TILES_PER_CHUNK, S.TILE, S.CHUNK)
    assert S.TILES_PER_CHUNK * S.TILE_BUCKET <= S.ORDER_BUCKET
    # the staging of the scan, and the block size of the score grid (the launch's, and emit_body's assumption)
    scan = (CSRC / "adsb_scan_fast.hip").read_text()
    assert re.search(r"constexpr int kHitCap = (\d+);", scan).group(1) == str(S.HIT_CAP)
    assert S.HIT_CAP < S.TILE_BUCKET
    aux = (CSRC / "adsb_aux.hip").read_text()
    rx = (CSRC / "adsb_score_rx.hip").read_text()
    for text, kernels in ((aux, ("k_score", "k_emit")), (rx, ("k_rx_adders", "k_score_rx", "k_emit_rx"))):
        for k in kernels:
            assert f"hipLaunchKernelGGL({k}, dim3(kScoreBlocks), dim3({S.SCORE_THREADS}), 0," in text, k
    assert "static_assert(kScoreBlocks == 256" in (CSRC / "adsb_score_dev.h").read_text()
    assert "scan[2][256]" in (CSRC / "adsb_score_dev.h").read_text() and "stage[5 * 256]" in (CSRC / "adsb_score_dev.h").read_text()
    # the cap: the context's expression and the two places that test a pass against it
    ctx = (CSRC / "adsb_context.cpp").read_text()
    assert "c->hits_cap = (uint32_t)(4096 + max_chunks * 1024);" in ctx
    assert "std::min<uint32_t>(c->hits_cap, 262144u)" in ctx
    tail = (CSRC / "adsb_tail_dev.h").read_text()
    assert "n <= p.score.cap" in tail and "nh <= p.score.cap" in tail
    assert "sl.device_scored && n <= c->score.cap" in (CSRC / "adsb_collect.cpp").read_text()
    assert [S.score_cap(mc) for mc in (17, 128, 251, 252, 256, 512)] == [21504, 135168, 261120, 262144, 262144, 262144]
    # dense mode: the thresholds the legs' ordinary passes rely on
    col = (CSRC / "adsb_collect.cpp").read_text()
    assert "n >= 8u * (size_t)sl.n_chunks" in col and "n < 2u * (size_t)sl.n_chunks" in col


def test_the_geometry_of_the_slots():
    for tile in range(S.TILES_PER_CHUNK):
        for q in range(S.SLOTS_PER_TILE):
            if tile == 0 and q == 0:
                with pytest.raises(AssertionError):
                    S.slot_sample(0, tile, q)
                continue
            s = S.slot_sample(0, tile, q)
            # a burst from sample s has its preamble at j = s + 325 .. 326; every trial of it lies in the tile
            assert (s + S.LEAD - 8) // S.TILE == tile == (s + S.LEAD + 8) // S.TILE and s + S.SLOT <= S.CHUNK
            assert S.tile_of(s) == tile
    assert S.slot_sample(3, 16, 22) == 3 * S.CHUNK + 16 * S.TILE - S.LEAD + S.SLOT_FIRST + 22 * S.SLOT
    # the patches fit their slots, and a template's frames never share one
    for q in range(S.SLOTS_PER_TILE):
        for patch in (S.strong_patch(q), S.faint_patch(q), S.reply_patch(q)):
            assert patch.shape == (S.SLOT, 2) and patch.any() and not patch[300:].any()
    at = [s for s, _ in S.template_frames(5, 160)]
    assert len(set(at)) == 160 and all(S.tile_of(s) < S.TEMPLATE_TILES for s in at)
    assert min(b - a for a, b in zip(sorted(at), sorted(at)[1:])) >= S.SLOT
    assert not {(b, t) for b, t, q in S.topup_places(4)} & {(b, t) for b in range(4) for t in range(S.TEMPLATE_TILES + 1)}


def test_per_and_rounds():
    assert [S.per_block(n) for n in (0, 1, 255, 256, 257, 65536, 65537, 65792, 131072, 131073, 262144)] == \
        [0, 1, 1, 1, 2, 256, 257, 257, 512, 513, 1024]
    assert [S.rounds(n) for n in (1, 256, 65536, 65537, 65792, 131072, 131073, 131328, 262144)] == [1, 1, 1, 2, 2, 2, 3, 3, 4]
    assert S.boundaries(0) == [] and S.boundaries(1) == [] and S.boundaries(256) == list(range(1, 256))
    assert S.boundaries(257) == list(range(2, 257, 2))              # per = 2: 129 blocks
    b = S.boundaries(65537)                                        # per = 257: a second round of one hit in every full block
    assert len(b) == 510 and b[:4] == [256, 257, 513, 514] and b[-1] == 65535
    b = S.boundaries(65536)
    assert b == list(range(256, 65536, 256))
    b = S.boundaries(131100)                                       # per = 513: three rounds
    assert b[:3] == [256, 512, 513] and S.rounds(131100) == 3


def test_choose_and_choose_slots_on_made_up_counts():
    counts = [5, 4, 3, 3, 4, 5, 4, 8, 4, 4, 5, 4, 3, 3, 4, 5, 4, 3, 3, 4, 5, 4, 3]
    for target in (0, 3, 31, 32, 33, 55, 56, 57, 72, sum(counts)):
        idx = S.choose(counts, target)
        assert idx is not None and sum(counts[i] for i in idx) == target and len(set(idx)) == len(idx)
    assert S.choose(counts, 1) is None and S.choose(counts, 2) is None and S.choose(counts, sum(counts) + 1) is None
    other = [4, 3, 3, 5, 4, 4, 3, 5, 4, 3, 3, 4, 5, 4, 3, 3, 4, 5, 4, 3, 3, 4, 5]
    reply = [4, 3, 3, 4, 5, 4, 3, 3, 4, 5, 4, 3, 3, 4, 10, 4, 3, 3, 4, 5, 4, 3, 3]
    opts = [[(counts[q], 0, ("strong", q)), (other[q], 0, ("faint", q)), (0, reply[q], ("reply", q))] for q in range(23)]
    val = {("strong", q): (counts[q], 0) for q in range(23)}
    val.update({("faint", q): (other[q], 0) for q in range(23)})
    val.update({("reply", q): (0, reply[q]) for q in range(23)})
    for accept in (lambda s, m: s == 57 and m == 0, lambda s, m: s + m == 56 and s <= 29 and m >= 8,
                   lambda s, m: s + m == 56 and s >= 36, lambda s, m: s + m == 57 and m >= 12, lambda s, m: s == 31 and m == 0):
        ids = S.choose_slots(opts, accept)
        assert ids is not None and len({q for _, q in ids}) == len(ids)          # one patch a slot
        assert accept(sum(val[i][0] for i in ids), sum(val[i][1] for i in ids))
    assert S.choose_slots(opts, lambda s, m: s + m == S.TILE_BUCKET + 8) is not None
    assert S.choose_slots(opts, lambda s, m: s + m > S.TILE_BUCKET + 8) is None   # (never far past the sub-bucket)
    assert S.choose_slots(opts, lambda s, m: s == 2) is None
    for salt in range(1, 6):
        left = S.without_slot(opts, salt)
        assert sum(1 for o in left if not o) == 1 and S.choose_slots(left, lambda s, m: s == 56 and m == 0) is not None


def test_settle_moves_the_wanted_sum_by_what_the_measurement_missed():
    # a "device" that finds one hit more than the sum in the first selection, two fewer in the second
    off = {0: 1, 1: -2}
    made, got = S.settle(lambda m: m[0] + off.get(m[1], 0), 56, lambda want, salt: (want, salt))
    assert got == 56 and made == (56, 3)                     # wanted 56 (got 57), 55 (got 53), 58 (got 58), 56
    made, got = S.settle(lambda want: (want + 1, want), 57, lambda want, salt: want, accept=lambda g: g[0] == 57)
    assert (made, got) == (56, (57, 56))
    # a sum that cannot be made is looked for around the target
    made, got = S.settle(lambda want: want, 2, lambda want, salt: want if want >= 3 else None, accept=lambda g: g >= 3)
    assert made == 3
    with pytest.raises(AssertionError):
        S.settle(lambda want: 2 * (want // 2), 33, lambda want, salt: want, tries=6)


def test_the_straddle_finder():
    # 600 hits, per = 3: groups of (2, 1, 3, 1) trials a position -- the pairs and triples that lie across a multiple of 3
    sizes = [2, 1, 3, 1] * 86
    pos = np.repeat(np.arange(len(sizes), dtype=np.uint64) + (7 << 24), sizes)[:600]
    assert S.per_block(600) == 3
    found = S.straddling_groups(pos)
    by_hand = []
    start = 0
    for size in sizes:
        first, last = start, min(600, start + size) - 1
        start += size
        if first >= 600:
            break
        by_hand += [(m, first, last) for m in range(first + 1, last + 1) if m % 3 == 0]
    assert found == by_hand and len(found) > 50 and all(g0 < m <= g1 for m, g0, g1 in found)
    # single trials never straddle; a pass of one round in one block has no boundary at all
    assert S.straddling_groups(np.arange(600, dtype=np.uint64)) == []
    assert S.straddling_groups(np.zeros(1, dtype=np.uint64)) == []
    # per = 257: the boundary between a block's first round and its one-hit second round, and the next block's start
    pos = np.arange(65537, dtype=np.uint64)
    pos[255], pos[257] = pos[256], pos[256]
    assert S.straddling_groups(pos) == [(256, 255, 257), (257, 255, 257)]


def test_the_message_layout_and_the_comparison():
    from dump1090_rs_amd import _lib
    from oracle import binding
    import ctypes as C
    assert S.MSG.itemsize == C.sizeof(_lib.AdsbMsg) == C.sizeof(binding.OrcMsg)
    for name, field in (("msg", "msg"), ("len", "len"), ("try_phase", "try_phase"), ("score", "score"), ("j", "j"), ("chunk", "chunk"),
                        ("signal_level", "level")):
        assert getattr(_lib.AdsbMsg, name).offset == getattr(binding.OrcMsg, name).offset == S.MSG.fields[field][1]
    a = np.zeros(5, dtype=S.MSG)
    a["j"] = np.arange(5)
    assert S.first_difference(a, a.copy()) is None
    for f, v in (("score", 1800), ("level", 1), ("chunk", 2), ("try_phase", 7)):
        b = a.copy()
        b[f][3] = v
        assert S.first_difference(a, b)[0] == 3
    b = a.copy()
    b["msg"][2, 13] = 1
    assert S.first_difference(a, b)[0] == 2
    assert S.first_difference(a, a[:4])[0] == 4 and S.first_difference(a[:0], a[:0]) is None


def test_the_oracle_lists_as_arrays(oracle_mod):
    """oracle_list / oracle_list_rx against the binding's own lists"""
    from dump1090_rs_amd import synth
    from tests import receivers_support as R
    iq = synth.make_iq(3 * S.CHUNK, n_bursts=40, seed=0x5C7, n_icao=5, df11_every=3)
    want = oracle_mod.Oracle().demod_iq(iq, threads=16)[0]
    got = S.oracle_list(oracle_mod.Oracle(), iq)
    assert len(got) == len(want) > 20
    import struct
    assert [(int(g["chunk"]), int(g["j"]), int(g["try_phase"]), int(g["score"]), bytes(g["msg"]), int(g["level"])) for g in got] == \
        [(w["chunk"], w["j"], w["try_phase"], w["score"], w["msg"], struct.unpack("<Q", struct.pack("<d", w["signal_level"]))[0]) for w in want]
    receivers = [0, 1, 0]
    model = R.Model(2).feed(iq, receivers)
    got = S.oracle_list_rx([oracle_mod.Oracle(), oracle_mod.Oracle()], iq, receivers)
    assert [(int(g["chunk"]), int(g["j"]), int(g["try_phase"]), int(g["score"]), bytes(g["msg"][: g["len"]])) for g in got] == \
        [k[:5] for k in model]
