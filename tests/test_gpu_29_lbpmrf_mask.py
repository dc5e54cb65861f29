"""bgs_lbpmrf_mask_device on the GPU against the fixture the reference's own MotionDetection::GetMotionsMaskHU made
(tests/golden/lbpmrf_mask_ref.npz) and, for small shapes, the numpy restatement (tests/lbpmrf_numpy.py).  Masks, labels and flows are
compared byte for byte; the sticky "did not converge" counter must read 0 after every test."""
import numpy as np
import pytest

import lbpmrf_numpy as ln
import lbpmrf_scenes as sc
from gpu_helpers import _torch
from tracking_amd import capi
from tracking_amd.engine import lbpmrf_mask_counters, lbpmrf_mask_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return np.load(sc.FIXTURE)


@pytest.fixture(autouse=True)
def converged():
    yield
    assert lbpmrf_mask_counters()[0] == 0, "a call did not converge within its launches"


def on_device(rates, rows, cols, **kw):
    torch = _torch()
    mask, labels, flow = lbpmrf_mask_device(torch.from_numpy(np.ascontiguousarray(rates, np.float32)).cuda(), rows, cols, **kw)
    torch.cuda.synchronize()
    return mask.cpu().numpy(), None if labels is None else labels.cpu().numpy(), None if flow is None else flow.cpu().numpy()


def check_case(ref, name):
    rows, cols, rates = sc.rates(name)
    assert int(ref[name + ".rate_crc"][0]) == sc.crc(rates)
    want_mask, want_labels, want_flow = sc.fixture_case(ref, name)
    mask, labels, flow = on_device(rates, rows, cols)
    assert flow.tolist() == want_flow.tolist(), name
    bad = [i for i in range(len(rates)) if not np.array_equal(labels[i], want_labels[i])]
    assert not bad, (name, "labels", bad)
    bad = [i for i in range(len(rates)) if not np.array_equal(mask[i], want_mask[i])]
    assert not bad, (name, "mask", bad)
    return rates, mask, labels, flow


@pytest.mark.parametrize("name", ["one_node", "6x8", "7x6", "5x40"])
def test_smallest_shapes(ref, name):
    rows, cols, rates = sc.rates(name)
    _, mask, labels, flow = check_case(ref, name)
    for i in range(len(rates)):  # and the restatement itself
        m, lab, f = ln.lbpmrf_mask(rates[i], rows, cols)
        assert np.array_equal(mask[i], m) and np.array_equal(labels[i], lab) and int(flow[i]) == f, (name, i)


def test_random_mixes_batched(ref):
    """about 50 maps in two batches; each batch mixes the three draws and a trivial image"""
    n = 0
    for name in ("mix_24x44", "mix_37x70"):
        rates, _, labels, _ = check_case(ref, name)
        per_image = labels.reshape(len(rates), -1).mean(1)
        assert (per_image == 1).any() and ((per_image > 0) & (per_image < 1)).any()  # trivial and hard images in one batch
        n += len(rates)
    assert n >= 50


@pytest.mark.parametrize("name", ["wide_70x264", "tall_134x136"])
def test_several_workgroups_both_ways(ref, name):
    check_case(ref, name)


def test_ladder(ref):
    """one unit has to cross a chain of 200 nodes; mirrored too, with a trivial image between the two"""
    _, _, labels, flow = check_case(ref, "ladder")
    assert (labels[0] == ln.SOURCE).sum() == 3 and labels[0][1, 0] == ln.SOURCE and labels[0][1, 1] == ln.SOURCE  # the two left chain nodes and the pendant of the second
    assert (labels[2] == ln.SOURCE).sum() == 4  # the mirror gains the pendant that the missing edges of column 0 deny the first map
    assert labels[1].all() and flow.tolist() == [399, 400, 399]


def test_extremes(ref):
    _, mask, labels, _ = check_case(ref, "extremes")
    assert not labels[0].any() and not mask[0].any()  # all rates 1.0
    assert labels[1].all() and mask[1].any()          # all rates 0.0
    assert labels[2][10, 10] == ln.SOURCE and mask[2][13, 22] == 255  # the island inside the ring is a filled hole
    assert labels[3].sum() == 1 and not mask[3].any()  # the speck


def test_duality_on_a_frame_too_large_for_the_restatement():
    rows, cols = 270, 480
    nh, nw = sc.nodes(rows, cols)
    rates = np.stack([sc.uniform(nh, nw, 77), sc.mostly_neutral(nh, nw, 78), sc.binary(nh, nw, 79), sc.blobs(nh, nw, 80)])
    mask, labels, flow = on_device(rates, rows, cols)
    for i in range(len(rates)):
        assert ln.duality(ln.sink_weights(rates[i]), labels[i]) == int(flow[i]), i
    assert 0 < labels[1].mean() < 1 and 0 < labels[3].mean() < 1
    assert set(np.unique(mask)) <= {0, 255}


def test_optional_outputs_leave_the_mask_unchanged():
    rows, cols, rates = sc.rates("mix_24x44")
    full = on_device(rates, rows, cols)
    for kw in ({"want_labels": False}, {"want_flow": False}, {"want_labels": False, "want_flow": False}):
        mask, labels, flow = on_device(rates, rows, cols, **kw)
        assert np.array_equal(mask, full[0]), kw
        assert labels is None or np.array_equal(labels, full[1])
        assert flow is None or np.array_equal(flow, full[2])


def test_a_single_map_without_the_batch_axis(ref):
    rows, cols, rates = sc.rates("wide_70x264")
    want_mask, want_labels, want_flow = sc.fixture_case(ref, "wide_70x264")
    mask, labels, flow = on_device(rates[0], rows, cols)
    assert mask.shape == (rows, cols) and np.array_equal(mask, want_mask[0]) and np.array_equal(labels, want_labels[0]) and flow.tolist() == [int(want_flow[0])]


@pytest.mark.parametrize("rows,cols,area", [(24, 45, 5), (24, 44, 4), (4, 4, 5)])
def test_refusals(rows, cols, area):
    torch = _torch()
    with pytest.raises(capi.BgsError) as e:
        lbpmrf_mask_device(torch.zeros((1, 1), dtype=torch.float32, device="cuda"), rows, cols, histogram_area=area)
    assert e.value.code == capi.ERR_UNSUPPORTED
