"""Frame files: the one place of the package that opens, lists, names and writes image files (host-side I/O, off the hot path).
Readers give uint8 [H,W,3] / [N,H,W,3]; writers take uint8 [V,H,W,3] and encode by Pillow or, with on_device, by evoworld_amd.png,
which is imported only there: a run that never asks for it never loads it.  numbered_paths is the name rule of every frame dump
(unified_loop_consistency.py:104-108,432-453)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MAX_DECODE_THREADS = 16


def _map(fn, items, threads=None):
    """[fn(x) for x in items] on `threads` threads (None: as many as allowed), never more than MAX_DECODE_THREADS or the host's CPUs"""
    threads = min(threads or MAX_DECODE_THREADS, MAX_DECODE_THREADS, os.cpu_count() or 1, len(items))
    if threads <= 1:
        return [fn(x) for x in items]
    with ThreadPoolExecutor(max_workers=threads) as pool:
        return list(pool.map(fn, items))


def pil_to_rgb(im):
    """a PIL image of any mode -> uint8 [H,W,3], a writable array of its own (torch.from_numpy takes it as it is)"""
    return np.array(im.convert("RGB"))


def decode_rgb(path, jpg_fallback=False):
    """image file -> uint8 [H,W,3].  jpg_fallback: a missing X.png is read from X.jpg if that exists (dataset/CameraTrajDataset.py:430-433)"""
    from PIL import Image
    alt = os.path.splitext(path)[0] + ".jpg"
    if jpg_fallback and not os.path.exists(path) and os.path.exists(alt):
        path = alt
    with Image.open(path) as im:
        return pil_to_rgb(im)


def list_images(folder, exts):
    """The sorted names under `folder` that end in one of `exts`.  The names are compared in lower case, so exts written in lower case,
    such as (".png", ".jpg"), find a.png and B.PNG alike; a caller that wants one case only filters the result."""
    return sorted(f for f in os.listdir(folder) if f.lower().endswith(tuple(exts)))


def stack_frames(arrays, device, first_file):
    """equal-sized uint8 [H,W,3] arrays -> uint8 [N,H,W,3] on `device`; ValueError naming `first_file` when the sizes differ"""
    shapes = {a.shape for a in arrays}
    if len(shapes) > 1:
        raise ValueError(f"images of one batch differ in size ({sorted(shapes)}), first file {first_file}")
    return torch.from_numpy(np.stack(arrays)).to(device)


def read_frames(paths, device, threads=None):
    """image files (at least one) -> uint8 [N,H,W,3] on `device`, in path order, decoded on `threads` threads as _map bounds them"""
    paths = list(paths)
    return stack_frames(_map(decode_rgb, paths, threads), device, paths[0])


def numbered_paths(dir, n, start=0, first=1, digits=3, ext=".png"):
    """dir/NNN.png for n frames: the number is index + start + first, zero-padded to at least `digits` (a longer number is not cut).
    first=1, digits=3 names the frame dumps; first=0, digits=2 the memory panoramas 00.png .. 23.png."""
    return [os.path.join(dir, f"{i + start + first:0{digits}}{ext}") for i in range(n)]


def write_frames(paths, frames_u8, on_device=False, threads=None):
    """uint8 [V,H,W,3] (tensor or numpy array) -> one PNG file per path (ValueError when the counts differ), in directories made as needed.
    on_device: evoworld_amd.png encodes the device tensor (same pixels, other file bytes); otherwise Pillow, serially unless `threads`.
    Returns the paths."""
    paths = list(paths)
    for d in {os.path.dirname(p) for p in paths}:
        os.makedirs(d or ".", exist_ok=True)
    if on_device:
        from .png import write_png_files
        write_png_files(paths, frames_u8)
    else:
        from PIL import Image
        arr = frames_u8.cpu().numpy() if isinstance(frames_u8, torch.Tensor) else frames_u8
        _map(lambda pf: Image.fromarray(pf[1]).save(pf[0]), list(zip(paths, arr, strict=True)), threads or 1)
    return paths


def write_numbered(dir, frames_u8, start=0, on_device=False, first=1, digits=3):
    """numbered_paths + write_frames: the frames as dir/NNN.png.  Returns the paths."""
    return write_frames(numbered_paths(dir, len(frames_u8), start, first, digits), frames_u8, on_device)
