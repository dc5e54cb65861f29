"""The LbpMrf mask stage without a GPU: the numpy restatement against the fixture the reference's own
MotionDetection::GetMotionsMaskHU made (tests/golden/lbpmrf_mask_ref.npz), hand-checked patterns, the refusals of
bgs_lbpmrf_mask_check and the exported symbols.  Every comparison is byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import lbpmrf_numpy as ln
import lbpmrf_scenes as sc
from tracking_amd import capi

FIXTURE, fixture_case = sc.FIXTURE, sc.fixture_case


@pytest.fixture(scope="module")
def ref():
    return np.load(FIXTURE)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_restatement_equals_the_reference(ref, name):
    rows, cols, rates = sc.rates(name)
    assert int(ref[name + ".rate_crc"][0]) == sc.crc(rates), "the scene generator no longer makes the fixture's inputs"
    mask, labels, flow = fixture_case(ref, name)
    assert len(rates) == len(mask)
    for i, rate in enumerate(rates):
        m, lab, f = ln.lbpmrf_mask(rate, rows, cols)
        assert np.array_equal(lab, labels[i]), (name, i)
        assert f == int(flow[i]), (name, i)
        assert np.array_equal(m, mask[i]), (name, i)


def test_fixture_lists_every_case_and_reaches_every_branch(ref):
    assert list(ref["cases"]) == list(sc.CASES)
    assert all(int(v) > 0 for v in ref["branches"]), dict(zip(ref["branch_names"], ref["branches"]))


def labels_of(t, nh, nw):
    return ln.max_flow_labels(np.array(t, np.int64).reshape(nh, nw), nh, nw)


def test_single_node():
    # t = 0: the source's unit stays, the node is reachable; t >= 1: the sink takes it
    assert [(int(lab[0, 0]), f) for lab, f in (labels_of([t], 1, 1) for t in (0, 1, 8))] == [(ln.SOURCE, 0), (ln.SINK, 1), (ln.SINK, 1)]
    mask, labels, flow = ln.lbpmrf_mask(np.zeros((1, 1), np.float32), 5, 6)
    assert labels[0, 0] == ln.SINK and flow == 1
    assert mask.shape == (5, 6) and not mask.any()  # its pixel (row 3, column 3) does not survive the erosion


def test_node_0_0_is_isolated():
    # 3 x 3 nodes, every node hungry (t = 8) but (0, 0), which has excess: with an edge its unit would leave and (0, 0) would be SINK
    t = np.full((3, 3), 8)
    t[0, 0] = 0
    labels, flow = labels_of(t, 3, 3)
    assert labels[0, 0] == ln.SOURCE and labels.sum() == 8 and flow == 8


def test_row_0_has_no_horizontal_edges():
    # nodes (1, 0) and (2, 0) of a grid that is row 0 alone: excess beside room for 7.  An edge between them would carry the unit
    # and make (1, 0) SINK; there is none, so the unit stays and (1, 0) is SOURCE.
    t = np.array([[1, 0, 8, 1]])
    labels, flow = labels_of(t, 1, 4)
    assert labels.tolist() == [[1, 0, 1, 1]] and flow == 3
    # the same four nodes as row 1 of a two-row grid do exchange the unit
    t2 = np.array([[1, 1, 1, 1], [1, 0, 8, 1]])
    labels2, flow2 = labels_of(t2, 2, 4)
    assert labels2[1].tolist() == [1, 1, 1, 1] and flow2 == 8


def test_neutral_plateau_is_sink():
    # t = 1 everywhere: source and sink capacities cancel, nothing is reachable from the source
    labels, flow = labels_of(np.ones((6, 7)), 6, 7)
    assert labels.all() and flow == 42
    # and beside an excess node whose unit a far deficit takes: the plateau between them stays SINK but for the saturated path's tail
    t = np.ones((2, 6), np.int64)
    t[1, 1], t[1, 5] = 0, 8
    labels, flow = labels_of(t, 2, 6)
    assert labels.all() and flow == 12


def test_sink_weights_truncate_and_clamp():
    r = np.array([1.0, 0.9375, 0.875, 0.5, 0.0, 1.5, -5000.0, np.float32(1) - np.float32(1e-7)], np.float32)
    assert ln.sink_weights(r).tolist() == [0, 0, 1, 4, 8, 0, 32767, 0]


@pytest.mark.parametrize("rows,cols,area,why", [(24, 45, 5, "odd"), (24, 44, 4, "histogram_area"), (24, 44, 1, "histogram_area"), (4, 44, 5, "no node"),
                                                 (24, 5, 5, "no node"), (24, 4, 5, "no node")])
def test_check_refuses(rows, cols, area, why):
    rc = capi.lib().bgs_lbpmrf_mask_check(rows, cols, area, 8.0)
    assert rc == capi.ERR_UNSUPPORTED
    assert why in capi.lib().bgs_last_error().decode()
    with pytest.raises(ln.Unsupported):
        ln.geometry(rows, cols, area)


def test_check_refuses_a_weight_that_is_not_finite():
    assert capi.lib().bgs_lbpmrf_mask_check(24, 44, 5, float("nan")) == capi.ERR_UNSUPPORTED
    assert capi.lib().bgs_lbpmrf_mask_check(24, 44, 5, float("inf")) == capi.ERR_UNSUPPORTED


@pytest.mark.parametrize("rows,cols,area", [(5, 6, 5), (24, 44, 5), (1080, 1920, 5), (3, 4, 3), (20, 26, 7)])
def test_check_accepts(rows, cols, area):
    assert capi.lib().bgs_lbpmrf_mask_check(rows, cols, area, 8.0) == 0
    ln.geometry(rows, cols, area)


def test_new_symbols_are_exported():
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("bgs_lbpmrf_mask_check", "bgs_lbpmrf_mask_device", "bgs_lbpmrf_mask_counters"):
        assert hasattr(lib, name), name
        assert name in [n for n, _, _ in capi.SYMBOLS], name
