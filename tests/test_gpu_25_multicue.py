"""The model stage of SJN_MultiCueBGS (bgs_multicue) on the GPU against what the reference's own, unmodified
SJN_MultiCueBGS.cpp computed (tests/golden/multicue_ref.npz, read through tests/multicue_numpy.py; nothing here needs the reference
tree) and against the numpy restatement beyond the fixture.  Every comparison is byte for byte or bit for bit, and the sticky
"overflow" counter is 0 in every run."""
import functools

import numpy as np
import pytest

import multicue_numpy as mc
import multicue_scenes as sc
from gpu_helpers import _torch
from tracking_amd import capi
from tracking_amd.engine import MultiCueModel, multicue_xyz

pytestmark = pytest.mark.gpu


def params_of(p):
    return capi.multicue_default_params(**{k: p[k] for k in mc.FIELDS})


def device_run(p, scenes, ghost, update):
    """scenes: one [T][rows][cols][3] array per stream, all through the same scripted maps.  Returns (landmarks [D][S][rh][rw],
    confidences, one dict of state planes per stream)."""
    torch = _torch()
    S, T = len(scenes), len(scenes[0])
    train = p["training_period"] + 1
    lms, confs = [], []
    with MultiCueModel(params_of(p), n_streams=S) as m:
        for t in range(T):
            f = torch.from_numpy(np.stack([s[t] for s in scenes])).cuda()
            if t < train:
                m.train(f)
                continue
            lm, cf = m.landmark(f)
            lms.append(lm.cpu().numpy()), confs.append(cf.cpu().numpy())
            d = t - train
            m.update(torch.from_numpy(np.repeat(ghost[d][None], S, 0)).cuda(), ghost=True)
            m.update(torch.from_numpy(np.repeat(update[d][None], S, 0)).cuda(), ghost=False)
        states = [{k: m.state(k, s) for k in mc.PLANES} for s in range(S)]
    return np.array(lms), np.array(confs), states


@functools.lru_cache(maxsize=None)
def fixture_run(case):
    r = mc.load()[case]
    return device_run(r["params"], [r["frames"]], r["ghost"], r["update"])


FAST_12x16 = dict(mc.DEFAULTS, **mc.FAST, reduced_width=16, reduced_height=12)


@functools.lru_cache(maxsize=None)
def seeded(seed, rows=37, cols=53, rh=12, rw=16, T=30):
    """A scripted scene beyond the fixture: frames, maps, and the restatement's landmarks, confidences and state."""
    p = dict(FAST_12x16, reduced_width=rw, reduced_height=rh)
    train = p["training_period"] + 1
    frames = sc.frames_of("scripted", rows, cols, T, train, seed)
    ghost, boxes = sc.maps_of("scripted", rh, rw, T - train)
    update = np.array([sc.update_map_of(b, rh, rw) for b in boxes])
    m, lms, confs = mc.run(p, frames, ghost, update)
    return p, frames, ghost, update, lms, confs, m.state()


def same_state(got, want, where):
    for k in mc.PLANES:
        assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (where, k)


@pytest.mark.parametrize("case", mc.cases())
def test_matches_reference_fixture(case):
    r = mc.load()[case]
    lms, confs, states = fixture_run(case)
    st = states[0]
    assert st["overflow"][0] == 0
    bad = [d for d in range(len(lms)) if not np.array_equal(lms[d, 0], r["landmark"][d])]
    assert not bad, ("landmark maps differ at detecting frames", bad[:8])
    assert confs[:, 0].tobytes() == r["conf"].tobytes()
    assert st["count"][0] == r["count"]
    for k in mc.STATE_PLANES:
        assert mc.crc(st[k]) == r["plane_crc"][k], k
        if k in r["planes"]:
            assert st[k].tobytes() == r["planes"][k].tobytes(), k
    assert np.array_equal(st["landmark"], r["landmark"][-1].reshape(-1)) and st["conf"].tobytes() == r["conf"][-1].tobytes()


@pytest.mark.parametrize("seed,rows,cols,rh,rw", [(101, 37, 53, 12, 16), (102, 21, 30, 9, 11), (103, 64, 48, 17, 70)])
def test_matches_restatement_beyond_the_fixture(seed, rows, cols, rh, rw):
    p, frames, ghost, update, lms, confs, want = seeded(seed, rows, cols, rh, rw)
    glm, gcf, states = device_run(p, [frames], ghost, update)
    assert np.array_equal(glm[:, 0], lms) and gcf[:, 0].tobytes() == confs.tobytes()
    assert states[0]["overflow"][0] == 0
    same_state(states[0], want, seed)


def test_three_streams_in_one_object():
    """Three different scenes in one object against three single-stream runs (one of them the fixture's case)."""
    r = mc.load()["fast_12x16"]
    runs = [seeded(s) for s in (201, 202)]
    scenes = [r["frames"][:30], runs[0][1], runs[1][1]]
    ghost, update = r["ghost"][:25], r["update"][:25]
    assert np.array_equal(update, runs[0][3]) and np.array_equal(ghost, runs[0][2])  # the same script
    lms, confs, states = device_run(r["params"], scenes, ghost, update)
    assert np.array_equal(lms[:, 0], r["landmark"][:25]) and confs[:, 0].tobytes() == r["conf"][:25].tobytes()
    for s, run in enumerate(runs, 1):
        one_lm, one_cf, one_st = device_run(r["params"], [scenes[s]], ghost, update)
        assert np.array_equal(lms[:, s], one_lm[:, 0]) and confs[:, s].tobytes() == one_cf[:, 0].tobytes()
        assert np.array_equal(lms[:, s], run[4]) and confs[:, s].tobytes() == run[5].tobytes()
        same_state(states[s], one_st[0], s)
        same_state(states[s], run[6], s)
        assert states[s]["overflow"][0] == 0


def test_absorption_disabled_leaves_the_cache_books_empty():
    _, _, states = fixture_run("no_absorption")
    st = states[0]
    assert not st["tcache"].any() and not st["ccache"].any() and not st["tcnt"].any() and not st["ccnt"].any()
    assert (st["tref"] == -1).all() and (st["cref"] == -1).all()


def test_xyz_on_every_triple():
    torch = _torch()
    tri = np.stack(np.meshgrid(*(np.arange(256, dtype=np.uint8),) * 3, indexing="ij"), -1).reshape(-1, 3)
    got = multicue_xyz(torch.from_numpy(tri).cuda()).cpu().numpy()
    want = np.concatenate([mc.xyz_of(tri[i:i + (1 << 20)]) for i in range(0, len(tri), 1 << 20)])
    assert np.array_equal(got, want), np.nonzero((got != want).any(1))[0][:8]


def test_state_and_geometry_orderings():
    torch = _torch()
    p = dict(FAST_12x16)
    f = torch.zeros((1, 37, 53, 3), dtype=torch.uint8, device="cuda")
    um = torch.ones((1, 12, 16), dtype=torch.uint8, device="cuda")

    def code(call, *a, **kw):
        with pytest.raises(capi.BgsError) as e:
            call(*a, **kw)
        return e.value.code

    with MultiCueModel(params_of(p)) as m:
        assert code(m.landmark, f) == capi.ERR_STATE  # before training is complete
        assert code(m.update, um) == capi.ERR_STATE
        m.train(f)
        assert code(m.train, torch.zeros((1, 36, 53, 3), dtype=torch.uint8, device="cuda")) == capi.ERR_GEOMETRY
        for _ in range(p["training_period"] - 1):
            m.train(f)
        assert code(m.landmark, f) == capi.ERR_STATE  # one training frame short
        assert m.state("count")[0] == p["training_period"]
        m.train(f)
        assert m.state("count")[0] == p["training_period"] + 2  # the last training frame bumps the counter twice
        assert code(m.train, f) == capi.ERR_STATE  # a call after the (training_period + 1)-th
        assert code(m.update, um) == capi.ERR_STATE  # no landmark call yet
        assert code(m.landmark, torch.zeros((1, 37, 54, 3), dtype=torch.uint8, device="cuda")) == capi.ERR_GEOMETRY
        lm, conf = m.landmark(f, want_conf=False)
        want = np.zeros((12, 16), np.uint8)
        want[2:-2, 2:-2] = 125  # a constant scene: no texture on either side and the colour matches; the border stays 0
        assert conf is None and np.array_equal(lm[0].cpu().numpy(), want)
        m.update(um, ghost=True)
        m.update(um, ghost=True)  # the ghost update leaves the landmark in force
        m.update(um)
        assert code(m.update, um) == capi.ERR_STATE and code(m.update, um, ghost=True) == capi.ERR_STATE
        assert m.state("overflow")[0] == 0
