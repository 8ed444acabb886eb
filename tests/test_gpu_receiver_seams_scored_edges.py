"""Receiver seams scored on the device (include/adsb_hip.h, "Receiver seams, scored on the device") where
tests/test_gpu_receiver_seams_scored.py does not go: more than one block of buffers in k_seam_prefix (passes of 256, 257 and
260 buffers in a context of 260), receiver indices above 8 and above 12 bits out of 16384, buffers without an own hit inside
an ordered pass and a pass with no own hit at all, and kept own hits that move DOWN from buffer 0 on.  The inputs, and what
each is for (asserted on the CPU when it is built), are tests/seam_scored_edges_support.py's; the expectation is
tests/seam_support.py's SeamModel at tolerance 0, lists as RS.keys and filter tables slot for slot.  Every judged pass is
asserted to have been ordered, merged and scored on the device (all_taken).  Legs A, C and D run their input once more
under adsb_set_receiver_carry, where the host merges (merge_seam_records): the same lists, and the same counts of seam
records and of dropped own hits -- counts of hits, which the model, a list of messages, cannot see."""
import numpy as np
import pytest

from tests import receivers_support as RS
from tests import seam_scored_edges_support as E
from tests import seam_scored_support as SS
from tests import test_gpu_receiver_seams_scored as T

pytestmark = pytest.mark.gpu
CHUNK, N = SS.CHUNK, SS.N
ZERO, on_device, all_taken = T.ZERO, T.on_device, T.all_taken


class Edge(T.Combined):
    """T.Combined with a priming pass of the context's own size (max_chunks dense buffers, all receiver 0's), and the
    host merge's count of dropped own hits beside its count of seam records."""

    def __init__(self, n_receivers, mode="both", max_chunks=N):
        from dump1090_rs_amd import Context
        self.c = Context(0, max_chunks)
        self.n_receivers = n_receivers
        try:
            c = self.c
            c.set_receivers(n_receivers)
            if mode == "both":
                c.set_receiver_carry_scoring(True)
                assert c.get_receiver_carry_scoring() and c.get_receiver_carry() and c.get_receiver_scoring()
            elif mode == "carry":
                c.set_receiver_carry(True)
            else:
                assert mode == "scoring"
                c.set_receiver_scoring(True)
            d = on_device(E.tiled(max_chunks))
            c.demod_iq_device_rx(d.data_ptr(), max_chunks * CHUNK, np.zeros(max_chunks, dtype=np.uint32), cap=1 << 17)
            assert c.stats()["n_records"] >= 8 * max_chunks
            del d
            c.icao_flush()
            if mode != "scoring":
                c.receiver_carry_reset()
            self.mark()
        except BaseException:
            self.c.close()
            raise

    def now(self):
        return dict(super().now(), host_dropped=self.c.selftest_rx_seam_counters()["dropped"])


def run(s, inputs, maps, groups, dense=None):
    """Every group of passes submitted back to back, no flush anywhere, then collected.  -> the lists; s.steps: what the
    counters had moved by when each pass had been collected"""
    c = s.c
    got = []
    s.steps = getattr(s, "steps", [])
    for group in groups:
        devs = [on_device(inputs[k]) for k in group]
        for d, k in zip(devs, group):
            c.submit_iq_device_rx(d.data_ptr(), len(inputs[k]), maps[k])
        assert c.pending() == len(group)
        for k in group:
            got.append(RS.keys(c.collect(cap=1 << 17)))
            s.steps.append(s.since())
            if dense is None or k in dense:
                assert c.stats()["n_records"] >= 8 * len(maps[k]), k
        del devs
    return got


def tables_equal(c, model, receivers):
    for r in receivers:
        assert list(c.receiver_filter_table(r)) == model.table(r), r


def the_host_merge_agrees(n_receivers, max_chunks, inputs, maps, groups, dense, wants, device):
    """The same input under adsb_set_receiver_carry: the host merges and replays every pass.  The lists are the same, and
    so are the counts the model cannot see: seam records merged, own hits dropped."""
    with Edge(n_receivers, "carry", max_chunks) as s:
        assert run(s, inputs, maps, groups, dense) == wants
        host = s.since()
    print("host merge", host)
    assert host["merged_passes"] == 0 and host["taken"] == 0 and host["replays"] == len(maps), host
    assert host["host_seam_records"] == device["seam_records"], (host, device)
    assert host["host_dropped"] == device["dropped"], (host, device)


# ------------------------------------------------------------------------------------------------- leg A
@pytest.mark.parametrize("nb", [256, 257, 260])
def test_more_than_one_block_of_buffers(hip_lib, oracle_mod, nb):
    """Two passes of nb buffers back to back in a context of 260, six receivers: k_seam_prefix scans D and S 256 buffers a
    turn and carries both into the next -- 256 is one full block, 257 a second block with one member (a seam frame in
    front of buffer 256 in the first pass, a dropped edge hit in the second), 260 the whole context; 256 and 257 are also
    passes shorter than the context, ordered on the device.  A wrong carry makes the pass declare itself unscored: the
    lists would still be right, the counters say it.  (So they did of the host's room test, adds_have_room_rx, which took a
    receiver's thousands of repeated DF18 add() calls for as many values and refused both passes; it counts distinct
    values now.)"""
    maps, wants, model, planted = E.leg_a_case(nb)
    inputs = E.leg_a_inputs(nb)[0]
    with Edge(E.A_RECEIVERS, "both", E.A_CONTEXT) as s:
        got = run(s, inputs, maps, [[0, 1]])
        device = s.since()
        print("device merge", device)
        assert got == wants
        tables_equal(s.c, model, range(E.A_RECEIVERS))
        all_taken(s, 2)
        assert device["dropped"] >= len(planted["edge"])    # (found at j = 325 by the pass's own scan: each is dropped)
    the_host_merge_agrees(E.A_RECEIVERS, E.A_CONTEXT, inputs, maps, [[0, 1]], None, wants, device)


# ------------------------------------------------------------------------------------------------- leg B
@pytest.mark.parametrize("mode", ["both", "scoring"])
def test_receiver_indices_above_8_and_12_bits(hip_lib, oracle_mod, mode):
    """16384 receivers, of which 0, 1, 255, 256, 257, 4095, 4096, 16382 and 16383 are heard, four passes in flight: a
    receiver index cut to 8 bits (rx_key, the first-adder entry, a carry row, rx_map, the additions' receivers) makes 256
    hear what 0 heard, one cut to 12 bits 4096 -- the CPU has shown both lists to differ from the model's."""
    wants, model = E.leg_b_case(mode)
    inputs, maps, planted = E.leg_b_inputs()
    with Edge(E.B_RECEIVERS, mode) as s:
        c = s.c
        assert run(s, inputs, maps, [[0, 1, 2, 3]]) == wants
        tables_equal(c, model, E.B_USED)
        for r in E.B_UNUSED:
            assert not c.receiver_filter_table(r).any(), r
        if mode == "both":
            all_taken(s, 4)
        else:
            assert T.since_core(s.since()) == dict(ZERO, taken=4, rebuilds=1), s.since()


# ------------------------------------------------------------------------------------------------- leg C
def test_buffers_without_an_own_hit(hip_lib, oracle_mod):
    """All-zero buffers inside an ordered pass: buffer 0 (k_seam_mark's first hit fills own_start from 0), buffers 5, 6, 7
    (the hit behind the gap fills all three; 5 and 7 hold one seam record's message each, 6 nothing) and buffers 18, 19
    (the last hit fills up to the end; 19 holds a seam record's message).  A seam record of such a buffer lands at
    own_start[b] - D + S."""
    inputs, maps, wants, model = E.leg_c_gaps_case()
    with Edge(E.C_RECEIVERS) as s:
        assert run(s, inputs, maps, [[0, 1]]) == wants
        tables_equal(s.c, model, range(E.C_RECEIVERS))
        device = all_taken(s, 2)
        print("device merge", device)
    the_host_merge_agrees(E.C_RECEIVERS, N, inputs, maps, [[0, 1]], None, wants, device)


def test_a_pass_that_is_nothing_but_seams(hip_lib, oracle_mod):
    """A dense pass that ends every receiver's stream with a frame inside its last 326 samples and a pass of 20 all-zero
    buffers, submitted together (dense mode is decided when a pass is collected, so the silent pass is still ordered on the
    device): no own hit, k_seam_mark's n == 0 branch fills own_start, and the pass's three messages are its seam records.
    Both passes are merged, scored and taken from the device."""
    inputs, maps, wants, model, ends = E.leg_c_only_seams_case()
    warm, last = list(range(E.C_WARM)), [E.C_WARM, E.C_WARM + 1]
    with Edge(E.C_RECEIVERS) as s:
        assert run(s, inputs, maps, [warm]) == wants[:E.C_WARM]
        all_taken(s, E.C_WARM)
        before = s.since()
        assert run(s, inputs, maps, [last], dense=last[:1]) == wants[E.C_WARM:]
        tables_equal(s.c, model, range(E.C_RECEIVERS))
        device = all_taken(s, E.C_WARM + 2)
        print("device merge", before, device)
        assert device["seam_records"] - before["seam_records"] >= len(ends)
    the_host_merge_agrees(E.C_RECEIVERS, N, inputs, maps, [warm, last], warm + last[:1], wants, device)


# ------------------------------------------------------------------------------------------------- leg D
def test_own_hits_move_down_from_buffer_0(hip_lib, oracle_mod):
    """Buffer 0 of the judged pass drops an own hit (a DF17 at j = 325 that only a zero lead-in finds) and no seam frame
    is planted before buffer 8: own_shift is S - D = 0xFFFFFFFF in two's complement and every kept own hit of the first
    buffers moves down by one."""
    inputs, maps, wants, model = E.leg_d_case()
    with Edge(E.D_RECEIVERS) as s:
        assert run(s, inputs, maps, [[0, 1]]) == wants
        tables_equal(s.c, model, range(E.D_RECEIVERS))
        device = all_taken(s, 2)
        print("device merge", device)
        assert s.steps[1]["dropped"] - s.steps[0]["dropped"] >= 1      # (the judged pass's own)
    the_host_merge_agrees(E.D_RECEIVERS, N, inputs, maps, [[0, 1]], None, wants, device)
