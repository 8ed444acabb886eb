"""A coarse guard against a context that leaks as a whole: a large context with signal statistics, two receivers scored on
the device and a ring is created, used for one pass and destroyed nine times over, and the device's free memory does not
sink.  (The fine-grained check -- every single reservation, every failure path -- is tests/test_context_lifetime_cpu.py.)

F is what creating and enabling everything takes from the device's free memory.  Free memory after the eighth cycle may
not be below free memory after the second by more than F / 2; the first two cycles are the warm-up in which the runtime
keeps what it keeps.  Two idle readings taken before anything is created that differ by more than F / 2 mean other
tenants of the device are moving the number: the test fails saying so.  The ninth context's list, like every cycle's,
equals the CPU oracle's (one oracle per receiver, tests/receivers_support.py), at tolerance 0."""
import numpy as np
import pytest

from dump1090_rs_amd import synth
from tests import receivers_support as RS

pytestmark = pytest.mark.gpu
CHUNK = RS.CHUNK
N = 17   # the smallest context that scores on the device
CYCLES = 8


def free_bytes() -> int:
    import torch
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info(0)[0])


def open_context():
    from dump1090_rs_amd import Context
    c = Context(0, N)
    try:
        c.set_signal_stats(True)
        c.set_receivers(2)
        c.set_receiver_scoring(True)
        c.ring_create(N * CHUNK)
    except BaseException:
        c.close()
        raise
    return c


def test_create_use_destroy_cycles_do_not_sink_free_memory(hip_lib, oracle_mod):
    iq = synth.make_iq(N * CHUNK, n_bursts=N * 12, seed=1907, n_icao=40, df11_every=3)
    rx_map = (np.arange(N) % 2).astype(np.uint32)
    want = RS.Model(2).feed(iq, rx_map)
    assert len(want) >= N   # (the stream has something to decode for both receivers)

    def one_pass(c):
        got = RS.keys(c.demod_iq_rx(iq, rx_map, cap=1 << 16))
        assert len(c.signal_stats()) == N
        return got

    idle = [free_bytes(), free_bytes()]
    c = open_context()
    reserved = idle[1] - free_bytes()
    c.close()
    print(f"idle readings {idle}, F = {reserved} bytes")
    assert reserved > (8 << 20), reserved   # (bitmaps, lists and the ring's staging: tens of MB)
    assert abs(idle[0] - idle[1]) <= reserved // 2, \
        f"free device memory moved by {abs(idle[0] - idle[1])} bytes between two idle readings (F = {reserved}): other tenants are moving the number"

    after = []
    for _ in range(CYCLES):
        c = open_context()
        try:
            assert one_pass(c) == want
        finally:
            c.close()
        after.append(free_bytes())
    print("free after each cycle:", after)
    assert after[CYCLES - 1] >= after[1] - reserved // 2, (after, reserved)

    c = open_context()
    try:
        assert one_pass(c) == want
    finally:
        c.close()
