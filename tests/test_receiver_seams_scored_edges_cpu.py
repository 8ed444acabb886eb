"""The inputs of tests/test_gpu_receiver_seams_scored_edges.py, built and judged without a device: every builder of
tests/seam_scored_edges_support.py asserts, from the plant list and tests/seam_support.py's SeamModel, what its input is
for -- seam frames found with carry and not without on either side of buffer 256, buffers that hold nothing but a seam
frame, a dropped hit in front of the first seam record, lists that change when a receiver index is cut to 8 or 12 bits.
A change to synth or to F.fill_capture that empties a leg of its purpose fails here, on any machine."""
import pytest

from tests import seam_scored_edges_support as E


@pytest.mark.parametrize("nb", [256, 257, 260])
def test_leg_a_inputs(oracle_mod, nb):
    maps, wants, model, planted = E.leg_a_case(nb)
    assert [len(m) for m in maps] == [nb, nb] and len(wants) == 2
    assert all(planted[kind] for kind in E.SS.KINDS)


@pytest.mark.parametrize("mode", ["both", "scoring"])
def test_leg_b_inputs(oracle_mod, mode):
    wants, model = E.leg_b_case(mode)
    assert len(wants) == 4
    for r in E.B_USED:
        assert any(model.table(r)), r


def test_leg_c_gaps_input(oracle_mod):
    inputs, maps, wants, model = E.leg_c_gaps_case()
    assert E.X in model.table(0) and E.X not in model.table(1) and E.X not in model.table(2)


def test_leg_c_only_seams_input(oracle_mod):
    inputs, maps, wants, model, ends = E.leg_c_only_seams_case()
    assert len(wants[-1]) == len(ends) == E.C_RECEIVERS


def test_leg_d_input(oracle_mod):
    inputs, maps, wants, model = E.leg_d_case()
    assert 0x4D0001 not in model.table(int(maps[1][0]))
