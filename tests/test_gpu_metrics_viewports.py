"""-m gpu: the cube-face viewports of the metrics CLI (evoworld_amd.metrics.cube_viewports over reprojection.Equi2Pers /
ew_equi2pers): where each face looks, that a face is exactly the direct Equi2Pers call, what the planar metrics give on the faces, and
the CLI with --projection cube and with the ws_* metrics on a PNG tree.  None of this is in the reference."""
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_ref as MR
import ws_metrics_ref as WR

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, S = 64, 128, 32
FACES = ("front", "right", "back", "left", "up", "down")


def _coded_pano():
    """uint8 [H,W,3]: R codes the longitude quadrant centred on each side face (front around W/2, right around 3W/4, back around the
    seam, left around W/4), G the latitude band (top quarter, middle half, bottom quarter), B is constant"""
    y, x = np.mgrid[0:H, 0:W]
    quadrant = ((x + W // 8) // (W // 4)) % 4                       # 0: back (seam), 1: left, 2: front, 3: right
    band = np.where(y < H // 4, 0, np.where(y < 3 * H // 4, 1, 2))
    return np.stack([40 + 50 * quadrant, 30 + 90 * band, np.full_like(x, 200)], -1).astype(np.uint8)


def _clip(T, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([np.stack([128 + 100 * np.sin(0.07 * x * (c + 1) + 0.11 * y + 0.4 * t) for c in range(3)], -1) for t in range(T)])
    return np.clip(a + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)


def test_face_orientation():
    from evoworld_amd import metrics as M
    assert M.CUBE_FACES == FACES
    pano = _coded_pano()
    faces = M.cube_viewports(torch.from_numpy(pano)[None].to(DEV))
    assert faces.shape == (6, 1, S, S, 3) and faces.dtype == torch.uint8 and faces.is_cuda
    centre = faces[:, 0, S // 2, S // 2].cpu().numpy().astype(int)
    want = {"front": pano[H // 2, W // 2], "right": pano[H // 2, 3 * W // 4], "back": pano[H // 2, 0], "left": pano[H // 2, W // 4],
            "up": pano[0, W // 2], "down": pano[H - 1, W // 2]}
    assert len({tuple(v) for v in want.values()}) == 6                              # the code tells all six apart
    assert tuple(pano[H // 2, W - 1]) == tuple(pano[H // 2, 0])                     # the back face's centre: both sides of the seam
    for k, name in enumerate(FACES):
        assert np.abs(centre[k] - want[name].astype(int)).max() <= 1, (name, centre[k], want[name])


def test_faces_are_the_direct_equi2pers_calls():
    from evoworld_amd import metrics as M
    from evoworld_amd.reprojection import Equi2Pers
    clip = torch.from_numpy(_clip(3, 1)).to(DEV)
    rots = ({"yaw": 0.0}, {"yaw": -math.pi / 2}, {"yaw": math.pi}, {"yaw": math.pi / 2}, {"pitch": math.pi / 2}, {"pitch": -math.pi / 2})
    for size in (None, 20):
        faces = M.cube_viewports(clip, size)
        s = size or S
        assert faces.shape == (6, 3, s, s, 3) and faces.is_contiguous()
        for k, r in enumerate(rots):
            assert torch.equal(faces[k], Equi2Pers(s, s, 90).batch(clip, [r] * 3)), FACES[k]
    with pytest.raises(ValueError):
        M.cube_viewports(clip.float())


def _videos(faces):
    """uint8 [6,T,S,S,3] -> [6,T,3,S,S] in [0,1]: every face one video"""
    return faces.permute(0, 1, 4, 2, 3).float() / 255.0


def test_metrics_on_the_faces_of_identical_and_polar_differing_clips():
    from evoworld_amd import metrics as M
    a = _clip(2, 2)
    fa = M.cube_viewports(torch.from_numpy(a).to(DEV))
    same_p, same_s = M.calculate_psnr(_videos(fa), _videos(fa)), M.calculate_ssim(_videos(fa), _videos(fa))
    assert same_p["value_mean"] == 100 and abs(same_s["value_mean"] - 1.0) <= 1e-12
    for k in range(6):
        p, s = M.video_metrics_u8(fa[k], fa[k])
        assert (p == 100).all() and np.abs(s - 1.0).max() <= 1e-12
    # b differs from a only above 72 degrees north (rows y with (H/2 - y - 0.5) * 180 / H > 72, i.e. y <= 5): only `up` sees it -- a side
    # face of 90 degrees reaches 45 degrees of latitude at most, and `down` looks away
    b = a.copy()
    rows = [y for y in range(H) if (H / 2 - y - 0.5) * 180.0 / H > 72.0]
    assert rows == list(range(6))
    b[:, rows] = 255 - b[:, rows]
    fb = M.cube_viewports(torch.from_numpy(b).to(DEV))
    for k, name in enumerate(FACES):
        p, _ = M.video_metrics_u8(fa[k], fb[k])
        if name == "up":
            assert (p < 100).all(), p
        else:
            assert (p == 100).all() and torch.equal(fa[k], fb[k]), (name, p)


def _write_tree(root, gt, gen):
    for e in range(gt.shape[0]):
        for sub, v in (("predictions_gt_0", gt), ("predictions_0", gen)):
            d = os.path.join(root, f"ep_{e:03d}", sub)
            os.makedirs(d, exist_ok=True)
            for t in range(v.shape[1]):
                Image.fromarray(v[e, t]).save(os.path.join(d, f"{t + 1:03}.png"))


def _close(got, want, tol):
    got = json.loads(json.dumps(got))
    want = json.loads(json.dumps(want))
    assert got["video_setting"] == want["video_setting"] and got["video_setting_name"] == want["video_setting_name"]
    assert abs(got["value_mean"] - want["value_mean"]) <= tol
    for k in ("value", "value_std"):
        assert got[k].keys() == want[k].keys()
        assert max(abs(got[k][t] - want[k][t]) for t in got[k]) <= tol, k


def test_cli_cube_projection_and_ws_metrics_on_a_png_tree(tmp_path):
    from evoworld_amd import metrics as M
    gt = np.stack([_clip(12, 10), _clip(12, 11)])
    rng = np.random.default_rng(5)
    gen = np.clip(gt.astype(np.int16) + rng.integers(-12, 13, gt.shape), 0, 255).astype(np.uint8)
    _write_tree(str(tmp_path), gt, gen)
    argv = ["--data_path", str(tmp_path), "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0"]
    # cube: every (episode, face) is one video, episode-major
    M.main(argv + ["--projection", "cube", "--metrics", "psnr,ssim", "--result_file", "cube.json"])
    got = json.load(open(tmp_path / "cube.json"))
    assert list(got) == ["ssim", "psnr", "projection", "viewport_size", "not_computed"]
    assert got["projection"] == "cube" and got["viewport_size"] == S
    assert got["psnr"]["video_setting"] == got["ssim"]["video_setting"] == [12, 3, S, S]
    v1, v2 = (torch.cat([_videos(M.cube_viewports(torch.from_numpy(v[e]).to(DEV))) for e in range(2)]) for v in (gt, gen))
    assert v1.shape == (12, 12, 3, S, S)
    _close(got["psnr"], M.calculate_psnr(v1, v2), 1e-5)
    _close(got["ssim"], M.calculate_ssim(v1, v2), 1e-9)
    small, _ = M.main(argv + ["--projection", "cube", "--viewport_size", "24", "--metrics", "psnr"])
    assert list(small) == ["psnr", "projection", "viewport_size", "not_computed"] and small["viewport_size"] == 24
    assert list(small["psnr"]["video_setting"]) == [12, 3, 24, 24]
    with pytest.raises(ValueError, match="cube"):
        M.main(argv + ["--projection", "cube", "--metrics", "psnr,ws_psnr"])
    # the latitude-weighted metrics next to the planar ones, against the restatement
    M.main(argv + ["--metrics", "psnr,ssim,ws_psnr,ws_ssim", "--result_file", "ws.json"])
    ws = json.load(open(tmp_path / "ws.json"))
    assert list(ws) == ["ssim", "psnr", "ws_psnr", "ws_ssim", "not_computed"]
    assert set(ws["not_computed"]) == {"fvd", "lpips", "latent_mse", "loop_closure_latent_mse"}
    w = WR.latitude_weights(H)
    fa, fb = (MR.u8_values(v).transpose(0, 1, 4, 2, 3) for v in (gt, gen))
    setting = torch.Size([12, 3, H, W])
    _close(ws["ws_psnr"], M.aggregate([[WR.ws_psnr_ref(fa[e, t], fb[e, t], w) for t in range(12)] for e in range(2)], setting), 1e-5)
    _close(ws["ws_ssim"], M.aggregate([[WR.wssim_ref(fa[e, t], fb[e, t], w) for t in range(12)] for e in range(2)], setting), 1e-9)
    assert ws["ws_psnr"]["value_mean"] != ws["psnr"]["value_mean"]
    only, _ = M.main(argv + ["--metrics", "ws_ssim"])
    assert list(only) == ["ws_ssim", "not_computed"]
    # a default invocation is what it was
    plain, _ = M.main(argv + ["--result_file", "plain.json"])
    assert list(plain) == ["ssim", "psnr", "not_computed"] and plain["not_computed"] == M.NOT_COMPUTED
    assert json.load(open(tmp_path / "plain.json"))["psnr"] == ws["psnr"]
    with pytest.raises(ValueError, match="LPIPS"):
        M.main(argv + ["--metrics", "psnr,ws_lpips"])
