"""The first-adder table of device-side scoring, the part that needs no GPU: tests/score_hash_support.py restates the
table's size rule and home-slot formula, and tests/test_gpu_score_hash.py builds its colliding streams from that
restatement -- here it is held against the library's own inline functions (csrc/adsb_device.h: score_hash_size,
score_hash_slot), compiled into a small host program; the supply of addresses per home slot; and, on a model of the
table, that the streams' clusters do wrap from the last slot to slot 0 and are crossed by the strangers' lookups."""
import shutil
import subprocess

import numpy as np
import pytest

from tests import score_hash_support as H
from tests.conftest import ROOT

CSRC = ROOT / "dump1090_rs_amd" / "csrc"
MAX_CHUNKS = (17, 28, 29, 60, 61, 252, 512)
PROGRAM = r"""
#include <cstdio>
#include "adsb_device.h"
// lines of "s <cap>" -> score_hash_size(cap), "h <value>" -> score_hash_slot(value)
int main()
{
    char kind;
    unsigned long long x;
    while (std::scanf(" %c %llu", &kind, &x) == 2)
        std::printf("%u\n", kind == 's' ? adsb::score_hash_size((uint32_t)x) : adsb::score_hash_slot((uint32_t)x));
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_hash")
    src, exe = d / "score_hash_host.cpp", d / "score_hash_host"
    src.write_text(PROGRAM)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wextra",
                    "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)], check=True, cwd=d, capture_output=True, timeout=600)

    def ask(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, check=True)
        out = [int(x) for x in r.stdout.split()]
        assert len(out) == len(lines)
        return out
    return ask


def gpu_test_addresses():
    """every address the GPU tests use, with the max_chunks of the context it is used in"""
    out = []
    for mc, form in ((17, "small"), (29, "small"), (17, "large")):
        s = H.colliding_stream(mc, form)
        out += [(a, mc) for a in s.taught + s.strangers]
    s = H.colliding_stream(17, "small", fix=True)
    out += [(a, 17) for a in s.taught + s.strangers]
    for n in (2, 3):
        m = H.multi_capture(n)
        out += [(a, 17) for g in m.extra_taught for a in g]
    return out


def test_the_restatement_against_the_librarys_own_functions(program):
    # the size rule, at the context sizes where the table size changes and at its cap
    caps = [min(4096 + 1024 * mc, 262144) for mc in MAX_CHUNKS]
    assert program([f"s {c}" for c in caps]) == [H.hash_size(mc) for mc in MAX_CHUNKS]
    assert [H.hash_size(mc) for mc in MAX_CHUNKS] == [1 << 16, 1 << 16, 1 << 17, 1 << 17, 1 << 18, 1 << 19, 1 << 19]
    assert program(["s 0", "s 1", "s 2", "s 3", "s 32768", "s 32769"]) == [1, 2, 4, 8, 65536, 131072]
    # ... and where the context takes its argument from (the rule's other half, adsb_context.cpp)
    ctx = (CSRC / "adsb_context.cpp").read_text()
    assert "c->hits_cap = (uint32_t)(4096 + max_chunks * 1024);" in ctx
    assert "std::min<uint32_t>(c->hits_cap, 262144u)" in ctx and "score_hash_size(cd.cap)" in ctx
    # the home slot: ~10 000 values, the edges and every address of the GPU tests
    r = np.random.default_rng(0x5C0E)
    used = gpu_test_addresses()
    values = [0, 1, 0xFFFFFF, 0x100000, 0x800000] + [int(v) for v in r.integers(0, 1 << 24, size=9000)] + sorted({a for a, _ in used})
    assert 9000 <= len(values) <= 12000
    raw = program([f"h {v}" for v in values])
    for mc in MAX_CHUNKS:
        mask = H.hash_size(mc) - 1
        assert [x & mask for x in raw] == [H.home(v, mc) for v in values], mc
    assert all(x < 1 << 24 for x in raw)
    by_value = dict(zip(values, raw))
    for a, mc in used:
        assert by_value[a] & (H.hash_size(mc) - 1) == H.home(a, mc)
    # addresses_at is home()'s inverse
    for mc, slot in ((17, -1), (17, 0), (29, -2), (512, 5)):
        at = H.addresses_at(slot, mc)
        assert len(at) and all(H.home(int(a), mc) == slot % H.hash_size(mc) for a in at[:: max(1, len(at) // 50)])
        inside = {int(a) for a in at}
        assert [v for v in values if H.home(v, mc) == slot % H.hash_size(mc)] == [v for v in values if v in inside]


def test_every_home_slot_has_the_supply_the_construction_draws_from():
    assert H.supply(512) >= 23        # 2^19 slots
    assert H.supply(17) >= 255        # 2^16 slots
    # (addresses >= 0x100000 only: what is left at the homes the forms use covers the largest draw)
    for mc, form in ((17, "large"), (29, "small"), (17, "small")):
        for part in H.FORMS[form].values():
            for rel, n in part.items():
                assert int((H.addresses_at(rel, mc) >= 0x100000).sum()) >= 2 * n, (mc, form, rel)


def model_insert(table: dict, size: int, v: int, mc: int) -> int:
    """score_hash_insert's walk on a dict {slot: value}: the slot v ends up in"""
    h = H.home(v, mc)
    while h in table and table[h] != v:
        h = (h + 1) & (size - 1)
    table[h] = v
    return h


def model_lookup(table: dict, size: int, v: int, mc: int):
    """score_hash_first's walk: (found, slots visited)"""
    h, walked = H.home(v, mc), 1
    while h in table and table[h] != v:
        h = (h + 1) & (size - 1)
        walked += 1
    return h in table, walked


@pytest.mark.parametrize("mc, form", [(17, "small"), (29, "small"), (17, "large")])
def test_the_cluster_wraps_and_the_strangers_cross_it(mc, form):
    """The wrap case: on a model of the table, in any insertion order, the taught addresses occupy one run of slots that
    goes through the last slot into slot 0; keys sit in slots below their home (they went round); a stranger at the last
    home or at home 0 is looked up across occupied slots on both sides of the wrap and ends on an empty one.  A walk
    that took h + 1 without the mask would leave the table at exactly these keys."""
    s = H.colliding_stream(mc, form)
    size = H.hash_size(mc)
    assert len(s.taught) + len(s.strangers) <= 700 and len(s.taught) < 0.02 * size
    r = np.random.default_rng(7)
    for order in (list(s.taught), list(reversed(s.taught)), [s.taught[i] for i in r.permutation(len(s.taught))]):
        table: dict = {}
        slots = {v: model_insert(table, size, v, mc) for v in order}
        assert len(table) == len(s.taught) and len(set(slots.values())) == len(s.taught)
        first = min(H.home(v, mc) for v in s.taught if H.home(v, mc) > size // 2)
        run = [(first + k) & (size - 1) for k in range(len(s.taught))]
        assert set(table) == set(run) and run[0] > run[-1]                      # one cluster, through the wrap
        went_round = [v for v in s.taught if slots[v] < H.home(v, mc)]
        assert len(went_round) >= 20                                            # insertions that crossed slot S-1 -> 0
        moved = [v for v in s.taught if slots[v] != H.home(v, mc)]
        assert len(moved) >= len(s.taught) - 8                                  # (nearly nobody sits at home)
        for v in s.taught:
            assert model_lookup(table, size, v, mc)[0]
        crossing = 0
        for v in s.strangers:
            found, walked = model_lookup(table, size, v, mc)
            assert not found
            h = H.home(v, mc)
            if h >= size - 2 or h == 0:
                assert walked > run[-1] + 1                                     # ... through every occupied slot to the run's end
                crossing += h != 0
            elif h in table:
                assert walked > 1
            else:
                assert walked == 1                                              # in front of the cluster: the home is empty
        assert crossing >= 20
