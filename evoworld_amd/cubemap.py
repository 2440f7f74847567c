"""Folder tool for the panorama <-> cubemap conversions of Navigator (evoworld/inference/navigator_evoworld.py:514-864):

  python -m evoworld_amd.cubemap to-cubemap --input DIR --output DIR [--scale_factor 2] [--nearest] [--size W H]
      every NNN.png panorama of --input -> NNN_cubemap.png (the cross) and NNN_{right,left,top,bottom,front,back}.png.
      --size W H resizes frames that are not 2:1 (the model's 1024x576) first, with the Pillow-exact bilinear.
  python -m evoworld_amd.cubemap to-pano --input DIR --output DIR --size W H [--scale_factor 2]
      every NNN_{face}.png set of --input -> NNN.png, a W x H panorama.
  --device_png (either command) encodes the output files on the device (evoworld_amd.png) instead of by Pillow.

PNG decoding (and Pillow's encoding) runs on at most 16 threads (evoworld_amd.frames) and is streamed to the device one batch at a
time (as metrics.evaluate does); every batch is one launch per stage.
"""
import argparse
import os
import sys

from . import frames
from . import reprojection as RP

BATCH = 25
FACES = RP.CUBEMAP_FACE_NAMES


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m evoworld_amd.cubemap", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    a = sub.add_parser("to-cubemap", help="panoramas -> cross + six faces")
    a.add_argument("--input", required=True)
    a.add_argument("--output", required=True)
    a.add_argument("--scale_factor", type=int, default=2)
    a.add_argument("--nearest", action="store_true", help="nearest-neighbour sampling (interpolation=False)")
    a.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=None, help="resize to W x H (2:1) first, PIL bilinear")
    b = sub.add_parser("to-pano", help="six faces -> panorama")
    b.add_argument("--input", required=True)
    b.add_argument("--output", required=True)
    b.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), required=True)
    b.add_argument("--scale_factor", type=int, default=2)
    for p in (a, b):
        p.add_argument("--device_png", action="store_true", help="encode the output PNG files on the device")
    args = ap.parse_args(argv)
    if args.scale_factor < 1:
        ap.error("--scale_factor must be at least 1")
    return args


def _batches(items, n=BATCH):
    for i in range(0, len(items), n):
        yield items[i:i + n]


def _paths(folder, stems, suffix=""):
    return [os.path.join(folder, f"{s}{suffix}.png") for s in stems]


def panorama_stems(folder):
    """NNN of every NNN.png that is not itself an output of this tool"""
    return sorted(f[:-4] for f in frames.list_images(folder, (".png",)) if "_" not in f)


def face_stems(folder):
    """NNN of every complete NNN_{face}.png set"""
    files = set(os.listdir(folder))
    stems = sorted({f[:-len("_right.png")] for f in files if f.endswith("_right.png")})
    return [s for s in stems if all(f"{s}_{n}.png" in files for n in FACES)]


def to_cubemap(args, device="cuda"):
    stems = panorama_stems(args.input)
    if not stems:
        raise ValueError(f"no NNN.png panoramas under {args.input}")
    for batch in _batches(stems):
        x = frames.read_frames(_paths(args.input, batch), device)
        if args.size is not None:
            x = RP.resize_u8(x, args.size[1], args.size[0], "bilinear")
        cross, faces = RP.panorama_to_cubemap(x, not args.nearest, args.scale_factor)
        for name, frames_u8 in {"cubemap": cross, **faces}.items():
            frames.write_frames(_paths(args.output, batch, f"_{name}"), frames_u8, args.device_png, frames.MAX_DECODE_THREADS)
    return len(stems)


def to_pano(args, device="cuda"):
    stems = face_stems(args.input)
    if not stems:
        raise ValueError(f"no complete NNN_{{face}}.png sets under {args.input}")
    for batch in _batches(stems):
        faces = {n: frames.read_frames(_paths(args.input, batch, f"_{n}"), device) for n in FACES}
        pano = RP.cubemap_to_panorama(faces, args.size[0], args.size[1], args.scale_factor)
        frames.write_frames(_paths(args.output, batch), pano, args.device_png, frames.MAX_DECODE_THREADS)
    return len(stems)


def main(argv=None):
    args = parse_args(argv)
    n = to_cubemap(args) if args.command == "to-cubemap" else to_pano(args)
    print(f"cubemap {args.command}: {n} image(s) -> {args.output}", file=sys.stderr)
    return n


if __name__ == "__main__":
    main()
