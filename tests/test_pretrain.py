"""Host side of the detector's pre-training on rendered scenes (SPEC.md section 15, dtoid/pretrain.py): target selection
on a numpy SceneBatch at each threshold's edge, the object split with both fall-backs, the repeatability of the jitter
rows and of the set's draws, the refusals that come before the device is touched, and the kernel's place in the build.
No GPU."""
import numpy as np
import pytest
import torch

import ref_pretrain as rp
import ref_scene as rs
from ossid_code_amd import _build, pipeline, render, scenes
from ossid_code_amd.dtoid import pretrain

HW = (24, 41)
CAM_K = np.array([[40.0, 0.0, 20.0], [0.0, 40.0, 11.5], [0.0, 0.0, 1.0]])


def _atlas(ids=(1, 2, 3)):
    V, F = rs.cube(0.05)
    C = np.full((len(V), 3), 200, np.uint8)
    return scenes.MeshAtlas({o: render.Mesh(V, F, device="cpu", colors=C) for o in ids})


def _host_batch(gt_rows, instance_obj, scene_first):
    """A numpy SceneBatch whose gt_info is given; the images are blank (select_targets reads none)."""
    atlas = _atlas()
    I, S, (H, W) = len(instance_obj), len(scene_first) - 1, HW
    layout = scenes.Layout([atlas.index_of[o] for o in instance_obj], np.tile(np.eye(4), (I, 1, 1)), scene_first,
                           np.tile([40.0, 40.0, 20.0, 11.5], (S, 1)))
    info = np.zeros((I, 12), np.int32)
    info[:, :2] = gt_rows
    z = np.zeros((S, H, W), np.float32)
    return scenes.SceneBatch(atlas, layout, HW, np.zeros((S, H, W, 3), np.uint8), z, z, z.astype(np.uint16),
                             np.full((S, H, W), -1, np.int32), np.zeros((I, H, (W + 31) // 32), np.int32), info)


def test_select_targets_at_every_edge():
    T = scenes.TABLE_OBJ_ID
    #        (px_count_all, px_count_visib)                                                          kept?
    rows = [(984, 900),      # 0 the table of scene 0                                                 no
            (500, 0),        # 1 nothing visible                                                      no
            (420, 399),      # 2 one pixel under min_px                                               no
            (420, 400),      # 3 exactly min_px                                                       yes
            (1601, 400),     # 4 just under min_visib: 400 / 1601 < 0.25                              no
            (1600, 400),     # 5 exactly min_visib: 400 / 1600 == 0.25                                yes
            (984, 984),      # 6 the table of scene 1                                                 no
            (800, 800),      # 7 object 3, fully visible                                              yes
            (0, 0)]          # 8 nothing drawn at all: the fraction is 0, not a division by zero      no
    batch = _host_batch(rows, [T, 1, 2, 1, 2, 3, T, 3, 1], [0, 6, 9])
    got = pretrain.select_targets(batch)
    assert got.dtype == np.int32 and got.tolist() == [[0, 3], [0, 5], [1, 7]]                 # draw-list order
    assert pretrain.select_targets(batch, obj_ids=[3]).tolist() == [[0, 5], [1, 7]]
    assert pretrain.select_targets(batch, obj_ids=[2]).shape == (0, 2)
    assert pretrain.select_targets(batch, min_px=399).tolist() == [[0, 2], [0, 3], [0, 5], [1, 7]]
    assert pretrain.select_targets(batch, min_visib=400 / 1601).tolist() == [[0, 3], [0, 4], [0, 5], [1, 7]]
    assert pretrain.select_targets(batch, min_visib=0.0, min_px=0).tolist() == [[0, k] for k in range(1, 6)] + [[1, 7], [1, 8]]
    # the fraction is the one frames() reports
    fr = {(f["scene_id"], k): f["visib_fract"] for k, f in zip([1, 2, 3, 4, 5, 7, 8], batch.frames())}
    assert fr[0, 5] == 0.25 and fr[0, 4] < 0.25 and fr[1, 8] == 0.0


def test_split_objects_and_both_fallbacks():
    assert pretrain.split_objects([1, 2, 3, 4, 5, 8, 9]) == ([1, 2, 3, 5, 9], [4, 8], False)     # dtoid_dataset.py:38-39
    assert pretrain.split_objects([5, 1, 2]) == ([1, 2, 5], [1, 2, 5], True)                      # nothing to validate on
    assert pretrain.split_objects([8, 4]) == ([4, 8], [4, 8], True)                               # nothing to train on
    assert pretrain.split_objects(range(1, 16))[1] == [4, 8, 12]
    for bad in ([], [0, 1]):
        with pytest.raises(ValueError):
            pretrain.split_objects(bad)


def test_sample_jitter_repeats_and_keeps_its_ranges():
    a = pretrain.sample_jitter(64, np.random.default_rng(7), 1.0)
    b = pretrain.sample_jitter(64, np.random.default_rng(7), 1.0)
    c = pretrain.sample_jitter(64, np.random.default_rng(8), 1.0)
    assert a.dtype == np.float32 and a.shape == (64, 8)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and not np.array_equal(a.view(np.uint32), c.view(np.uint32))
    assert (a[:, :3] >= 0.7 * 0.9 - 1e-6).all() and (a[:, :3] <= 1.3 * 1.1 + 1e-6).all()
    assert (np.abs(a[:, 3:6]) <= 0.1).all() and (a[:, 6] >= 0).all() and (a[:, 6] <= 0.06).all()
    assert len(set(a.view(np.uint32)[:, 7].tolist())) > 60                          # 32-bit draws, kept as bits
    half = pretrain.sample_jitter(64, np.random.default_rng(7), 0.5)
    assert (np.abs(half[:, 3:6]) <= 0.05).all() and (half[:, 6] <= 0.03).all()
    none = pretrain.sample_jitter(3, np.random.default_rng(7), 0.0)
    assert np.array_equal(none[:, :7], np.tile(np.array([1, 1, 1, 0, 0, 0, 0], np.float32), (3, 1)))
    for bad in (lambda: pretrain.sample_jitter(0, np.random.default_rng(0)), lambda: pretrain.sample_jitter(4, 5),
                lambda: pretrain.sample_jitter(4, np.random.default_rng(0), 1.5)):
        with pytest.raises(ValueError):
            bad()


def test_the_restated_exponential_is_an_exponential():
    """ref_pretrain.device_exp writes out the device library's chain (SPEC 15.2). It is within one unit in the last place of
    the correctly rounded value everywhere a heat map can take it, exact at 0, and correct into the subnormals."""
    x = -np.random.default_rng(0).uniform(0.0, 740.0, 2000)
    x[:4] = [0.0, -1e-300, -744.0, -709.5]
    got, want = rp.device_exp(x), np.exp(x)
    ulps = np.abs(got.view(np.int64) - want.view(np.int64))
    assert ulps.max() <= 1 and got[0] == 1.0 and got[2] == want[2] > 0
    assert 0.0 < (ulps != 0).mean() < 0.2                  # the two are not the same function: the test's reason to exist
    assert rp.heatmap((3.0, 2.0, 5.0, 4.0, 1.0), 5, 7, 1.0)[3, 4] == 1.0 and not rp.heatmap(rp.EMPTY_BOX, 5, 7, 1.0).any()


def _bank(ids, n_views=12):
    """A TemplateBank filled by hand on the host: distinct constant images per (object, view), the level-0 view grid."""
    bank = pipeline.TemplateBank()
    quats = np.stack([pipeline._rotmat_to_quat(R) for R in render.view_grid(0)])
    for o in ids:
        bank.img[o] = torch.arange(n_views, dtype=torch.float32).reshape(-1, 1, 1, 1).expand(n_views, 3, 4, 4) / 100.0 + o
        bank.mask[o] = torch.ones(n_views, 1, 4, 4)
        bank.quats[o] = quats
    return bank


def _set(seed, **kw):
    atlas = _atlas()
    return pretrain.ScenePretrainSet(atlas, _bank([1, 2, 3]), CAM_K, HW, 3, 4, 2, seed, **kw)


def test_the_sets_draws_repeat_under_one_seed():
    """The host half of a refresh: layouts, sensor, then the shuffle, the template choice and the jitter rows."""
    targets = np.array([[s, 4 * s + k] for s in range(4) for k in (1, 2, 3)], np.int32)       # instance 4 s is scene s's table
    plans = []
    for seed in (3, 3, 4):
        st = _set(seed)
        layout, sensor = st.draw_targets()
        plans.append((layout.transforms, sensor.thresholds) + st.plan(layout, targets))
    a, b, c = plans
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[2], c[2])
    tr, _thr, tg, gidx, lidx, objs, jit = a
    assert sorted(map(tuple, tg.tolist())) == sorted(map(tuple, targets.tolist())) and not np.array_equal(tg, targets)
    assert jit.shape == (12, 8) and gidx.shape == lidx.shape == (12,)
    st = _set(3)
    for (s, i), o, g, l in zip(tg, objs, gidx, lidx):
        first = st._first[int(o)]
        assert first <= g < first + 12 and first <= l < first + 12
        assert l - first == st.bank.nearest_views(int(o), tr[i][:3, :3])[0]               # the single closest view
    assert _set(3, jitter=None).plan(scenes.sample_layouts(_atlas(), 4, 3, CAM_K, HW, np.random.default_rng(0)), targets)[4] is None


def test_refusals_come_before_the_device():
    rows = [(984, 900), (500, 450)]
    batch = _host_batch(rows, [scenes.TABLE_OBJ_ID, 1], [0, 2])
    ok = np.array([[0, 1]], np.int32)
    cases = {"not a batch": lambda: pretrain.scene_batch(object(), ok),
             "targets [T,3]": lambda: pretrain.scene_batch(batch, np.zeros((1, 3), np.int32)),
             "T = 0": lambda: pretrain.scene_batch(batch, np.zeros((0, 2), np.int32)),
             "heat map size": lambda: pretrain.scene_batch(batch, ok, heatmap_hw=(5, 0)),
             "jitter rows": lambda: pretrain.scene_batch(batch, ok, jitter=np.zeros((2, 8), np.float32)),
             "host arrays": lambda: pretrain.scene_batch(batch, ok),
             "select: not a batch": lambda: pretrain.select_targets(None),
             "set: batch size": lambda: pretrain.ScenePretrainSet(_atlas(), _bank([1, 2, 3]), CAM_K, HW, 3, 4, 0, 0),
             "set: foreign object": lambda: _set(0, obj_ids=[9]),
             "set: no templates": lambda: pretrain.ScenePretrainSet(_atlas(), _bank([1, 2]), CAM_K, HW, 3, 4, 2, 0),
             "set: jitter": lambda: _set(0, jitter=2.0)}
    for name, call in cases.items():
        with pytest.raises(ValueError):
            call()
        print("refused:", name)


def test_the_kernel_is_part_of_the_build_and_refuses_bad_sizes(hiplib):
    """csrc/pretrain.hip is one of build()'s sources, compiled for gfx950 like the rest, and the header declares its entry
    point; the entry point refuses before it launches (no device is needed to be refused)."""
    assert "pretrain.hip" in _build.SOURCES and any(s.endswith("pretrain.hip") for s in _build.sources())
    assert "--offload-arch=gfx950" in _build.FLAGS and "-ffp-contract=off" in _build.FLAGS
    assert "ossid_scene_dtoid_batch" in hiplib.exported_symbols()
    f = hiplib.fn("ossid_scene_dtoid_batch")
    p = 4096                                                    # never dereferenced: every call below is refused first

    def call(S=2, H=24, W=41, I=3, T=1, hh=5, hw=7, sigma=rp.SIGMA, color=p, out=p):
        return f(color, p, p, S, H, W, I, p, T, None, hh, hw, sigma, out, p, p, p, None)
    bad = [call(T=0), call(S=0), call(H=0), call(W=-1), call(I=0), call(hh=0), call(hw=0), call(sigma=0.0),
           call(H=1 << 15, W=1 << 15), call(color=None), call(out=None)]
    assert bad == [hiplib.EINVAL] * len(bad) and hiplib.EINVAL == -22
