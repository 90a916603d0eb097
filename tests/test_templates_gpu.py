"""Templates from a vertex-coloured mesh (SPEC.md 7.13-7.14) on the device: render.render_templates against the
restatement tests/ref_raster_color.py rendered through the same virtual cameras, the framing, and the TemplateBank /
DtoidNet wiring."""
import numpy as np
import pytest
import torch

import ref_raster as rr
import ref_raster_color as rc
from ossid_code_amd import synth

pytestmark = pytest.mark.gpu

T_SIZE, SS, PAD, DIST = 124, 4, 1.1, 0.8


@pytest.fixture(scope="module")
def colored():
    from ossid_code_amd import render
    V, F = rr.bump_mesh(2)
    C, _k = rc.axis_colors(V)
    return V, F, C, render.Mesh(V, F, colors=C)


def test_render_templates_equals_the_restatement(hiplib, colored):
    from ossid_code_amd import render
    V, F, C, mesh = colored
    img, mask, info = render.render_templates(mesh, cam_K=synth.CAM_K, views_per_call=32)
    img2, mask2, info2 = render.render_templates(mesh, cam_K=synth.CAM_K, views_per_call=162)
    assert img.shape == (162, 3, 124, 124) and mask.shape == (162, 1, 124, 124) and img.is_cuda
    assert img.dtype == mask.dtype == torch.float32
    assert torch.equal(img, img2) and torch.equal(mask, mask2) and np.array_equal(info["intrinsics"], info2["intrinsics"])
    R = render.view_grid(2)
    assert np.array_equal(info["rotations"], R) and info["quats"].shape == (162, 4) and info["template_z"].shape == (162,)
    # SPEC 7.14: the device's float64 framing against numpy's, then the float32 cast the kernel is given
    want, wtz = rc.framing(V.astype(np.float32), R, DIST, synth.CAM_K, T_SIZE, SS, PAD)
    cams64, tz = render._frame_views(mesh.vertices, R, DIST, synth.CAM_K, SS * T_SIZE, T_SIZE, PAD, 0.05)
    assert np.abs(cams64 / want - 1.0).max() < 1e-9 and np.abs(tz / wtz - 1.0).max() < 1e-9
    assert info["intrinsics"].dtype == np.float32                 # the cast: half an ulp of float32, 2^-24 relative
    assert np.abs(info["intrinsics"].astype(np.float64) / cams64 - 1.0).max() <= 2.0 ** -24 + 1e-12
    assert np.abs(info["template_z"] / tz - 1.0).max() < 1e-12
    img_h, mask_h = img.cpu().numpy(), mask.cpu().numpy()
    ring = int(np.floor((T_SIZE / 2.0) * (1.0 - 1.0 / PAD)))
    assert ring == 5
    for v in range(162):
        wi, wm = rc.template(V, F, C, R[v], DIST, info["intrinsics"][v], T_SIZE, SS)
        assert np.array_equal(img_h[v], wi) and np.array_equal(mask_h[v], wm), v
        m = mask_h[v, 0]
        assert m.any() and m.min() >= 0 and m.max() <= 1 and np.array_equal(m * 16, np.rint(m * 16))
        assert not img_h[v][:, m == 0].any()
        inner = m[ring:T_SIZE - ring, ring:T_SIZE - ring]
        assert m.sum() == inner.sum(), v                            # the outer ring is empty
        ys, xs = np.nonzero(inner)
        assert min(ys.min(), xs.min(), inner.shape[0] - 1 - ys.max(), inner.shape[1] - 1 - xs.max()) <= 2, v
    # other sizes go through the same path
    img3, mask3, info3 = render.render_templates(mesh, rotations=R[:5], size=31, supersample=2, cam_K=synth.CAM_K)
    for v in range(5):
        wi, wm = rc.template(V, F, C, R[v], DIST, info3["intrinsics"][v], 31, 2)
        assert np.array_equal(img3[v].cpu().numpy(), wi) and np.array_equal(mask3[v].cpu().numpy(), wm)


def test_template_bank_from_a_mesh(hiplib, colored):
    from ossid_code_amd import dtoid, pipeline, render
    V, F, C, mesh = colored
    bank = pipeline.TemplateBank()
    info = bank.add_mesh(7, mesh, cam_K=synth.CAM_K)
    R = info["rotations"]
    assert bank.img[7].shape == (162, 3, 124, 124) and bank.mask[7].shape == (162, 1, 124, 124)
    assert np.array_equal(bank.template_z[7], info["template_z"]) and np.array_equal(bank.quats[7], info["quats"])
    for v in range(162):
        assert bank.nearest_views(7, R[v])[0] == v
    assert 0 <= bank.train_view(7, R[3], np.random.default_rng(0)) < 162
    limg, lmask = bank.all_local(7)
    assert limg.shape == (160, 3, 124, 124) and lmask.shape == (160, 1, 124, 124)
    assert len(set(bank.test_views(7).tolist())) == 160
    # template_z, on its own: pred_z = (T / size) * -template_z as dtoid/model.py forms it, for the object seen at Z.
    # A tight box is at most the symmetric extent 2 m d / Z and at least half of it: pad Z <~ pred_z <~ 2 pad Z.
    for Z in (0.6, 1.0):
        poses = np.tile(np.eye(4), (162, 1, 1))
        poses[:, :3, :3], poses[:, 2, 3] = R, Z
        seen = render.render_depth(mesh, poses, synth.CAM_K, (480, 640)) > 0
        cols, rows = seen.any(1).cpu().numpy(), seen.any(2).cpu().numpy()
        for v in range(162):
            xs, ys = np.nonzero(cols[v])[0], np.nonzero(rows[v])[0]
            size = max(xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
            pred_z = (T_SIZE / size) * -bank.template_z[7][v]
            assert PAD * Z * 0.9 <= pred_z <= 2 * PAD * Z * 1.1, (v, Z, pred_z)
    # the detector takes the rendered views (random weights: nothing is claimed about what it finds)
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R[40], (0.05, -0.03, 0.7)
    color, depth = render.render_color(mesh, pose, synth.CAM_K, (480, 640))
    assert int((depth > 0).sum()) > 1000 and color[depth > 0].any()
    frame = (color.permute(2, 0, 1).to(torch.float32) / 255.0)[None].contiguous()
    torch.manual_seed(0)
    det = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda().eval()
    with torch.no_grad():
        det.model.classification.output.weight.normal_(0, 0.05)
        det.model.regression.output.weight.normal_(0, 0.01)
    out = det.forwardTestTime({"img": frame, "obj_id": torch.tensor([7]), "limg": limg[None], "lmask": lmask[None],
                               "template_z_values": torch.from_numpy(bank.template_z[7][bank.test_views(7)])[None]})
    k = out["pred_scores"].shape[0]
    assert k >= 1 and out["pred_bbox"].shape == (k, 4) and torch.isfinite(out["pred_bbox"]).all()
    assert torch.isfinite(out["pred_scores"]).all()
    assert (out["pred_template_ids"] >= 0).all() and (out["pred_template_ids"] < 160).all()
