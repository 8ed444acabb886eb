"""A short seeded soak of "many receivers, one pass" (include/adsb_hip.h): a few hundred random sequences over every
entry point that takes a map -- blocking from the host and resident, submit / collect at random depths, the ring, their
CU8 twins -- mixed with plain calls (every buffer is receiver 0), flushes of one receiver and of all, changes of the
number of receivers and of the threshold of the pooled replay, on the two context sizes of tests/test_gpu_receivers.py.
Everything against one CPU oracle per receiver (tests/receivers_support.py), tolerance 0, the filter tables included."""
import numpy as np
import pytest

from tests import receivers_support as RS

pytestmark = pytest.mark.gpu
CHUNK = RS.CHUNK


def quantise(iq):
    return np.ascontiguousarray(np.clip(np.rint(iq / 256.0 + 127.4), 0, 255).astype(np.uint8))


class Soak:
    def __init__(self, c, fmt, seed):
        import torch
        self.c, self.fmt = c, fmt
        self.rng = np.random.default_rng([0x50A4, seed])
        cs16, _ = RS.batch(3, 8)
        self.total = len(cs16) // CHUNK
        self.raw = {"cs16": cs16, "cu8": quantise(cs16)}
        self.meant = {"cs16": cs16, "cu8": np.ascontiguousarray(c.u8_table()[self.raw["cu8"].reshape(-1, 2)])}
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in self.raw.items()}
        torch.cuda.synchronize()
        self.bps = {"cs16": 4, "cu8": 2}
        self.n_receivers = 0
        self.model = None
        self.expected = []          # the lists of the passes in flight, in submission order
        self.ops = {}
        self.messages = 0
        (c.ring_create_u8 if fmt == "cu8" else c.ring_create)(min(c.max_chunks, 17) * CHUNK)

    def count(self, what):
        self.ops[what] = self.ops.get(what, 0) + 1

    def window(self, most):
        """(first buffer, buffers, samples cut off the end, map)"""
        r = self.rng
        n = int(r.integers(1, min(most, 6) + 1)) if r.random() < 0.85 else int(r.integers(1, most + 1))
        a = int(r.integers(0, self.total - n + 1))
        cut = int(r.integers(1, CHUNK)) if r.random() < 0.25 else 0
        few = r.random() < 0.3     # (a pass dominated by one or two receivers)
        m = r.integers(0, min(2, self.n_receivers) if few else self.n_receivers, size=n).astype(np.uint32)
        return a, n, cut, m

    def feed(self, fmt, a, n, cut, m):
        return self.model.feed(self.meant[fmt][a * CHUNK:(a + n) * CHUNK - cut], m)

    def collect_one(self):
        got = RS.keys(self.c.collect(cap=1 << 17))
        assert got == self.expected.pop(0), ("collect", self.ops)
        self.messages += len(got)

    def drain(self):
        while self.expected:
            self.collect_one()
        assert self.c.pending() == 0

    def tables(self):
        self.drain()
        for r in range(self.n_receivers):
            assert list(self.c.receiver_filter_table(r)) == self.model.table(r), (r, self.ops)
        self.count("tables")

    def set_receivers(self):
        self.drain()
        n = int(self.rng.choice([1, 2, 3, 5, 9]))
        if n != self.n_receivers:
            self.c.set_receivers(n)      # (a change restarts every receiver from an empty filter)
            self.n_receivers, self.model = n, RS.Model(n)
        self.count("set_receivers")

    def step(self):
        c, r = self.c, self.rng
        what = r.choice(["blocking", "blocking", "submit", "submit", "submit", "ring", "plain", "flush_one", "flush_one",
                         "flush_all", "collect", "tables", "set_receivers", "tune"])
        if what == "blocking":
            self.drain()
            fmt = "cu8" if r.random() < 0.3 else "cs16"
            a, n, cut, m = self.window(self.total)      # (longer than max_chunks: cut into passes)
            want = self.feed(fmt, a, n, cut, m)
            k = n * CHUNK - cut
            if r.random() < 0.5:
                part = self.raw[fmt][a * CHUNK:a * CHUNK + k]
                got = (c.demod_iq_rx_u8 if fmt == "cu8" else c.demod_iq_rx)(part, m, cap=1 << 17)
            else:
                ptr = self.dev[fmt].data_ptr() + self.bps[fmt] * a * CHUNK
                got = (c.demod_iq_device_rx_u8 if fmt == "cu8" else c.demod_iq_device_rx)(ptr, k, m, cap=1 << 17)
            assert RS.keys(got) == want, (what, fmt, a, n, cut, self.ops)
            self.messages += len(want)
        elif what == "submit":
            for _ in range(int(r.integers(1, c.max_in_flight() + 3))):
                if c.pending() == c.max_in_flight() or (self.expected and r.random() < 0.2):
                    self.collect_one()
                if r.random() < 0.15:
                    self.flush_one()
                fmt = "cu8" if r.random() < 0.3 else "cs16"
                a, n, cut, m = self.window(min(c.max_chunks, 17 + int(r.integers(0, 4))))
                self.expected.append(self.feed(fmt, a, n, cut, m))
                ptr = self.dev[fmt].data_ptr() + self.bps[fmt] * a * CHUNK
                (c.submit_iq_device_rx_u8 if fmt == "cu8" else c.submit_iq_device_rx)(ptr, n * CHUNK - cut, m)
        elif what == "ring":
            for _ in range(int(r.integers(1, 5))):
                if c.pending() == c.max_in_flight():
                    self.collect_one()
                a, n, cut, m = self.window(min(c.max_chunks, 17))
                self.expected.append(self.feed(self.fmt, a, n, cut, m))
                buf = c.ring_acquire_u8() if self.fmt == "cu8" else c.ring_acquire()
                k = n * CHUNK - cut
                buf[:k] = self.raw[self.fmt][a * CHUNK:a * CHUNK + k]
                c.ring_submit_rx(k, m)
        elif what == "plain":
            self.drain()
            a, n, cut, _ = self.window(self.total)
            want = self.feed("cs16", a, n, cut, np.zeros(n, dtype=np.uint32))
            assert RS.keys(c.demod_iq(self.raw["cs16"][a * CHUNK:(a + n) * CHUNK - cut], cap=1 << 17)) == want, (what, self.ops)
        elif what == "flush_one":
            self.flush_one()
        elif what == "flush_all":
            c.icao_flush()
            self.model.flush()
        elif what == "collect":
            if self.expected:
                self.collect_one()
        elif what == "tables":
            self.tables()
        elif what == "set_receivers":
            self.set_receivers()
        elif what == "tune":
            self.drain()
            c.selftest_rx_tune(int(r.choice([0, 1, 200])))
        self.count(what)

    def flush_one(self):
        k = int(self.rng.integers(0, self.n_receivers))
        self.c.icao_flush_receiver(k)
        self.model.flush(k)
        self.count("flush_receiver")


@pytest.mark.parametrize("max_chunks, fmt, seed", [(4, "cs16", 1), (4, "cu8", 2), (20, "cs16", 3), (20, "cu8", 4)])
def test_seeded_soak_of_every_rx_entry_point(hip_lib, oracle_mod, max_chunks, fmt, seed):
    """50 random sequences of four steps per case (200 in all), each ending with every receiver's filter table."""
    from dump1090_rs_amd import Context
    with Context(0, max_chunks) as c:
        s = Soak(c, fmt, seed)
        s.set_receivers()
        for _ in range(50):
            for _ in range(4):
                s.step()
            s.tables()
        assert s.messages > 5000, s.messages
        assert {str(k) for k in s.ops} >= {"blocking", "submit", "ring", "plain", "flush_one", "flush_all", "flush_receiver", "collect",
                                           "tables", "set_receivers", "tune"}, s.ops
        if max_chunks > 16:
            assert c.selftest_rx_counters()["pooled_passes"] > 0
