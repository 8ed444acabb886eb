"""The demodulator's exact ties and thresholds without a GPU (tests/edges_support.py): the streams and the edge-frame
catalogue are what they claim to be, the numpy model of the gates agrees with the oracle on them and on the reference
captures, and every edge the GPU tests lean on is reached often enough that those tests cannot pass vacuously."""
import numpy as np
import pytest

from tests import edges_support as E

IQ_STREAMS = ["debruijn", "low", "wide", "odd", "full", "catalogue", "planted"]
# per-edge floors over the IQ streams, about half of what they reach (measured: every tie cell >= 6, 7049 tie flips in
# all, 2*sig == 3*noise sliced 209, 3*noise - 2*sig == 1 65, loud == high >= 134 per residue of sum % 4, loud == high - 1
# 900, D == 0 >= 29 550 per slicer phase at 4185 sliced positions)
FLOORS = {**{k: 3 for k in E.COUNTER_KEYS if k.startswith("tie_flip")}, "snr_eq_sliced": 100, "snr_short1": 40,
          "loud_eq_r0": 100, "loud_eq_r1": 100, "loud_eq_r2": 100, "loud_eq_r3": 100, "loud_m1": 100,
          **{"d0_ph%d" % ph: 10000 for ph in range(5)}, "d0_cand": 2000}


@pytest.fixture(scope="module")
def stage(oracle_mod):
    """{stream: (iq, oracle stage lists)}"""
    return {name: (iq, oracle_mod.stage_lists(iq)) for name, iq in ((n, E.iq_stream(n)) for n in IQ_STREAMS)}


def test_magnitude_inverse_reaches_every_value_but_1_and_5(oracle_mod):
    ok = E.reachable()
    assert np.nonzero(~ok)[0].tolist() == [1, 5]
    want = np.nonzero(ok)[0]
    got = E._mags_of(E.mag_inverse()[want].astype(np.int64))
    assert np.array_equal(got, want)
    assert all(E.mag_inverse()[k].tolist() == [k // 2, 0] for k in (0, 2, 4, 100, 32766))
    with pytest.raises(ValueError):
        E.to_iq(np.array([0, 2, 5]))


def test_debruijn_walk_realises_every_comparison_pattern(oracle_mod):
    m, seq = E.debruijn_stream()
    assert len(seq) == 3 ** E.ORDER + E.ORDER - 1
    # the walk's signs are the sequence
    whole = E.walk(seq)
    assert np.array_equal(np.sign(np.diff(whole)), np.array([1, 0, -1])[seq])
    assert whole.min() >= 0 and whole.max() <= 65535
    # every pattern of p0..p13 in the buffers the demodulator sees (the buffers overlap by 19 samples)
    seen = np.zeros(3 ** E.ORDER, dtype=bool)
    for b in range(len(m) // E.CHUNK):
        x = m[b * E.CHUNK:(b + 1) * E.CHUNK]
        n = len(x) - E.ORDER
        s = 1 - np.sign(np.diff(x)).astype(np.int64)         # 0: "<", 1: "=", 2: ">"
        code = np.zeros(n, dtype=np.int64)
        for k in range(E.ORDER):
            code = 3 * code + s[k:k + n]
        seen[code] = True
    assert seen.all(), int((~seen).sum())
    # and the walk survives the IQ round trip
    iq = E.to_iq(m[:E.CHUNK])
    data, n = oracle_mod.Oracle().to_mag(iq)
    assert np.array_equal(data[E.LEAD:E.LEAD + n], m[:E.CHUNK])


@pytest.mark.parametrize("name", IQ_STREAMS)
def test_model_equals_the_oracle_stage_by_stage(stage, name):
    iq, sl = stage[name]
    for b, d in enumerate(sl["mags"]):
        n = min(E.CHUNK, len(iq) - b * E.CHUNK)
        m = E.stage_lists(d, n, b)
        for k in ("preamble", "snr", "cand"):
            assert [x for x in sl[k] if x >> 32 == b] == m[k], (name, b, k)


def test_model_equals_the_oracle_on_the_reference_captures(oracle_mod, fixture_iq):
    for name, iq in fixture_iq.items():
        sl = oracle_mod.stage_lists(iq)
        m = E.stage_lists(sl["mags"][0], len(iq))
        assert (sl["preamble"], sl["snr"], sl["cand"]) == (m["preamble"], m["snr"], m["cand"]), name
        assert len(m["cand"]) > 50


def test_model_equals_the_oracle_on_caller_magnitudes(oracle_mod):
    """Values no IQ pair reaches (1, 5, 65534 on the axis) and a non-zero lead-in: the model's candidates are the
    positions the oracle's demodulate2400 slices."""
    for name, seed in (("caller", 5), ("caller_full", 6)):
        mags = E.alphabet_stream(name, 1, seed)
        d = E.data_of(mags, lead=E.alphabet_stream(name, 1, seed + 10)[:E.LEAD])
        _, st = oracle_mod.Oracle().demodulate2400(d, E.CHUNK)
        g = E.gates(d, E.CHUNK)
        assert (st.preamble_pass, st.snr_pass, st.quiet_pass) == (
            int((g["branch"] >= 0).sum()), int(g["snr"].sum()), int(g["cand"].sum())), name
        assert st.quiet_pass > 100 and g["cand"][:E.LEAD].any()


def test_every_edge_is_reached(stage):
    tot = {}
    for name, (iq, sl) in stage.items():
        for b, d in enumerate(sl["mags"]):
            tot = E.add_counters(tot, E.counters(d, min(E.CHUNK, len(iq) - b * E.CHUNK)))
    short = {k: (tot[k], v) for k, v in FLOORS.items() if tot[k] < v}
    assert not short, short
    # and the pattern stage's "<=" superset differs from the reference where a tie changes the verdict
    assert sum(tot[k] for k in tot if k.startswith("tie_flip")) > 3000


def test_catalogue_twins_have_opposite_verdicts(oracle_mod):
    """Each case and its twin differ by one unit in one sample; the oracle finds the slot's frame at the case's
    position in exactly one of them, and in the one the model lets through."""
    cases = E.catalogue()
    kinds = {c.kind for c in cases}
    assert kinds == {"tie", "snr_eq", "snr_short1", "loud", "p12_p13", "slice"}
    names = {c.name.split("_", 1)[1].rsplit("_n", 1)[0] for c in cases if c.kind == "slice"}
    assert names == {"ph%d_bit%d" % (ph, b) for ph in range(5) for b in (0, 1)}    # every phase, bit 0 and 1
    mags, at = E.catalogue_mags(cases, E.CHUNK)
    iq = E.to_iq(mags)
    orc = oracle_mod.Oracle()
    orc.icao_flush()
    data, n = orc.to_mag(iq)
    assert np.array_equal(data[E.LEAD:E.LEAD + n], mags)
    found, _ = orc.demodulate2400(data, n)
    hit = {(w["j"] - E.LEAD, w["buffer"]) for w in found}
    g = E.gates(data, n)
    for i, c in enumerate(cases):
        t = cases[c.twin]
        assert t.twin == i and t.kind == c.kind
        diff = np.nonzero(c.mags != t.mags)[0]
        assert len(diff) == 1 and abs(int(c.mags[diff[0]]) - int(t.mags[diff[0]])) == 1, c.name
        present = (at[i], c.frame) in hit
        assert present == c.passes, c.name
        assert bool(g["cand"][E.LEAD + at[i]]) == (c.passes or c.kind == "slice"), c.name
        assert c.passes != t.passes, c.name
    # slicer cases: the sliced bit really is D == 0 in the winning trial
    for i, c in enumerate(cases):
        if c.kind == "slice" and not c.name.endswith("/twin"):
            n_bit = int(c.name.split("_n")[1])
            D, ph = E.slice_values(data, np.array([E.LEAD + at[i]]))
            assert D[0, c.tp - 4, n_bit] == 0 and ph[0, c.tp - 4, n_bit] == int(c.name.split("_ph")[1][0])


def test_cu8_table_realises_an_alphabet(oracle_mod):
    """The widening table of the GPU test (T[b] = 25 b) maps bytes {0, 2, 3, 4, 6} on the real axis onto the
    magnitudes {0, 100, 150, 200, 300} exactly."""
    t = cu8_table()
    b = cu8_stream(1, seed=3)
    wide = t[b.reshape(-1, 2)]
    data, n = oracle_mod.Oracle().to_mag(wide)
    want = 2 * 25 * b[:, 0].astype(np.int64)
    assert np.array_equal(data[E.LEAD:E.LEAD + n], want)
    assert set(np.unique(want).tolist()) == set(E.ALPHABETS["wide"])


def cu8_table() -> np.ndarray:
    return (25 * np.arange(256)).astype(np.int16)


def cu8_stream(n_buffers: int, seed: int) -> np.ndarray:
    """(N, 2) uint8 [re, im] with re from {0, 2, 3, 4, 6} and im = 0."""
    r = np.random.default_rng(seed)
    b = np.zeros((n_buffers * E.CHUNK, 2), dtype=np.uint8)
    b[:, 0] = np.array([0, 2, 3, 4, 6], dtype=np.uint8)[r.integers(0, 5, len(b))]
    return b
