"""-m "not gpu": evoworld_amd/frames.py, the reader, the writer and the name rule of every frame file, on the CPU (device="cpu", Pillow's
encoder).  PNG is lossless and nothing here computes: every comparison is exact."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as C
from evoworld_amd import frames

H, W = 12, 20
FRAMES = np.stack([C.texture(H, W, s) for s in range(3)])
FRAMES.setflags(write=False)


def _names(paths):
    return [os.path.basename(p) for p in paths]


def test_decode_rgb_every_mode_and_the_jpg_fallback(tmp_path):
    rgb = Image.fromarray(FRAMES[0])
    rgba = rgb.copy()
    rgba.putalpha(Image.fromarray(C.gradient(H, W)[:, :, 0]))
    for name, im in (("rgb", rgb), ("rgba", rgba), ("palette", rgb.quantize(16)), ("grey", rgb.convert("L"))):
        path = str(tmp_path / f"{name}.png")
        im.save(path)
        with Image.open(path) as back:
            assert back.mode == im.mode
            want = np.asarray(back.convert("RGB"))
        got = frames.decode_rgb(path)
        assert got.dtype == np.uint8 and got.shape == (H, W, 3) and np.array_equal(got, want), name
        assert np.array_equal(frames.pil_to_rgb(im), want), name
    assert np.array_equal(frames.decode_rgb(str(tmp_path / "rgb.png")), FRAMES[0])
    a = frames.pil_to_rgb(rgb)
    a[0, 0, 0] ^= 1                                                             # writable: torch.from_numpy takes it without a warning
    assert torch.from_numpy(a).shape == (H, W, 3)
    rgb.save(str(tmp_path / "only.jpg"), quality=95)
    with Image.open(tmp_path / "only.jpg") as back:
        want = np.asarray(back.convert("RGB"))
    assert np.array_equal(frames.decode_rgb(str(tmp_path / "only.png"), jpg_fallback=True), want)
    assert np.array_equal(frames.decode_rgb(str(tmp_path / "rgb.png"), jpg_fallback=True), FRAMES[0])      # an existing .png is itself
    with pytest.raises(FileNotFoundError):
        frames.decode_rgb(str(tmp_path / "only.png"))
    with pytest.raises(FileNotFoundError):
        frames.decode_rgb(str(tmp_path / "neither.png"), jpg_fallback=True)


def test_read_frames_order_threads_and_unequal_sizes(tmp_path, monkeypatch):
    order = [2, 0, 1, 2, 1, 0, 0]                                               # path order, not name order; more files than one thread takes
    paths = []
    for k, s in enumerate(order):
        paths.append(str(tmp_path / f"{9 - k}.png"))
        Image.fromarray(FRAMES[s]).save(paths[-1])
    one = frames.read_frames(paths, "cpu", threads=1)
    pooled = frames.read_frames(paths, "cpu")
    four = frames.read_frames(paths, "cpu", threads=4)
    assert one.dtype == torch.uint8 and one.shape == (len(order), H, W, 3) and one.device.type == "cpu"
    assert torch.equal(one, torch.from_numpy(FRAMES[order])) and torch.equal(one, pooled) and torch.equal(one, four)
    sizes = []

    class Pool(frames.ThreadPoolExecutor):                                      # the one pool: what it is opened with
        def __init__(self, max_workers):
            sizes.append(max_workers)
            super().__init__(max_workers=max_workers)

    monkeypatch.setattr(frames, "ThreadPoolExecutor", Pool)
    many = paths * 5                                                            # 35 files: more than MAX_DECODE_THREADS
    assert torch.equal(frames.read_frames(many, "cpu"), one.repeat(5, 1, 1, 1)) and torch.equal(frames.read_frames(many, "cpu", threads=1000), one.repeat(5, 1, 1, 1))
    assert torch.equal(frames.read_frames(paths[:2], "cpu", threads=4), one[:2]) and torch.equal(frames.read_frames(many, "cpu", threads=1), one.repeat(5, 1, 1, 1))
    cpus = os.cpu_count() or 1
    assert frames.MAX_DECODE_THREADS == 16 and sizes == ([min(16, cpus), min(16, cpus), 2] if cpus > 1 else [])     # one thread opens no pool
    odd = str(tmp_path / "odd.png")
    Image.fromarray(C.texture(H + 1, W)).save(odd)
    for threads in (1, None):
        with pytest.raises(ValueError) as e:
            frames.read_frames(paths[:2] + [odd], "cpu", threads=threads)
        assert paths[0] in str(e.value) and "differ in size" in str(e.value)


def test_numbered_paths(tmp_path):
    d = str(tmp_path)
    assert frames.numbered_paths(d, 3, start=24) == [os.path.join(d, n) for n in ("025.png", "026.png", "027.png")]
    assert _names(frames.numbered_paths(d, 3, first=0, digits=2)) == ["00.png", "01.png", "02.png"]
    wide = _names(frames.numbered_paths(d, 100, digits=2))
    assert wide[0] == "01.png" and wide[98:] == ["99.png", "100.png"]          # widened, not truncated
    assert _names(frames.numbered_paths(d, 2, ext=".jpg")) == ["001.jpg", "002.jpg"]
    assert frames.numbered_paths(d, 0) == []
    for start in (0, 24, 998):                                                  # the rule the dumps were written with
        assert _names(frames.numbered_paths(d, 3, start)) == [f"{i + start + 1:03}.png" for i in range(3)]


def test_write_frames_by_pillow(tmp_path):
    def back(paths):
        return np.stack([np.asarray(Image.open(p)) for p in paths])

    a = [str(tmp_path / "new" / "deeper" / f"{k}.png") for k in range(3)]       # neither directory exists
    frames.write_frames(a, FRAMES)
    assert np.array_equal(back(a), FRAMES)
    b = [str(tmp_path / "tensor" / f"{k}.png") for k in range(3)]
    frames.write_frames(b, torch.from_numpy(FRAMES.copy()))
    c = [str(tmp_path / f"pool{k % 2}" / f"{k}.png") for k in range(3)]         # two directories in one call
    frames.write_frames(c, FRAMES, threads=4)
    for pa, pb, pc in zip(a, b, c):
        assert open(pa, "rb").read() == open(pb, "rb").read() == open(pc, "rb").read()
    with pytest.raises(ValueError):
        frames.write_frames(a[:2], FRAMES)
    got = frames.write_numbered(str(tmp_path / "n"), FRAMES, 24)
    assert _names(got) == ["025.png", "026.png", "027.png"] == sorted(os.listdir(tmp_path / "n")) and np.array_equal(back(got), FRAMES)
    got = frames.write_numbered(str(tmp_path / "m"), FRAMES, first=0, digits=2)
    assert _names(got) == ["00.png", "01.png", "02.png"] and np.array_equal(back(got), FRAMES)
    assert open(got[1], "rb").read() == open(a[1], "rb").read()


def test_frames_does_not_import_the_device_encoder():
    kept = {k: sys.modules.pop(k) for k in ("evoworld_amd.png", "evoworld_amd.frames") if k in sys.modules}
    try:
        fresh = importlib.import_module("evoworld_amd.frames")
        assert fresh is not frames
        assert "evoworld_amd.png" not in sys.modules                            # a run that never asks for on_device never loads it
        assert not any(getattr(v, "__name__", "") in ("evoworld_amd.ops", "evoworld_amd.png", "torch.cuda") for v in vars(fresh).values())
    finally:
        sys.modules.pop("evoworld_amd.frames", None)
        sys.modules.update(kept)
    import evoworld_amd
    evoworld_amd.frames = frames                                                # the package attribute back to the module everyone holds


def test_list_images_as_the_callers_one_liners(tmp_path):
    for n in ("a.png", "B.PNG", "c.jpg", "d.jpeg", "e.txt", "001_right.png"):
        (tmp_path / n).write_bytes(b"")
    d = str(tmp_path)
    ls = os.listdir(d)
    # video encode; mvs cloud; png encode: the three sets that are passed, matched whatever the case of the name
    assert frames.list_images(d, (".png",)) == sorted(n for n in ls if n.lower().endswith(".png")) == ["001_right.png", "B.PNG", "a.png"]
    assert frames.list_images(d, (".png", ".jpg")) == sorted(f for f in ls if f.lower().endswith((".png", ".jpg"))) \
        == ["001_right.png", "B.PNG", "a.png", "c.jpg"]
    assert frames.list_images(d, (".png", ".jpg", ".jpeg")) == sorted(n for n in ls if n.lower().endswith((".png", ".jpg", ".jpeg"))) \
        == ["001_right.png", "B.PNG", "a.png", "c.jpg", "d.jpeg"]
    assert frames.list_images(d, [".jpeg"]) == ["d.jpeg"]                       # any sequence of suffixes
    # the dataset's rule on top of it: lower-case .png only
    assert [f for f in frames.list_images(d, (".png",)) if f.endswith(".png")] == sorted(f for f in ls if f.endswith(".png")) \
        == ["001_right.png", "a.png"]
    # the cubemap tool's rules on top of it
    from evoworld_amd import cubemap
    assert cubemap.panorama_stems(d) == sorted(f[:-4] for f in ls if f.lower().endswith(".png") and "_" not in f) == ["B", "a"]
    assert cubemap.face_stems(d) == []                                          # 001 has one face of six
