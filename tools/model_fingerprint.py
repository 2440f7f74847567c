"""Fingerprint of what the Python model layer hands to the library: for a refactor of unet.py / vae.py / clip.py the document this prints
must not change.  Run it on both commits (one process each) and compare the two JSON documents.

Per case (small U-Net with fused and unfused level-0 feed-forwards, the tiny U-Net with fp8 q/k/v, the tiny VAE, the tiny CLIP):
  weights   number of packed tensors found by walking model.w, and one sha256 over the sorted list of their per-tensor sha256 (dtype, shape,
            bytes): key names and order do not matter;
  launches  number of library calls, and
  trace     sha256 over them in order: wrappers set on the library object (the call path tests/test_gpu_call_path.py pins) record the
            entry name plus, for the two struct entry points, every integer / float field and one null bit per pointer field, for the
            others the integer / float positional arguments (pointers and the stream are left out);
  output    sha256 of the result bytes.
Only API that predates the shared model shell is used.   python tools/model_fingerprint.py [--out FILE] [--detail-dir DIR]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from evoworld_amd import _lib  # noqa: E402

DEV = "cuda"


def tensor_hashes(w):
    out = []

    def walk(v):
        if isinstance(v, torch.Tensor):
            t = v.detach().contiguous().cpu()
            out.append(hashlib.sha256(f"{t.dtype} {tuple(t.shape)} ".encode() + t.view(torch.uint8).numpy().tobytes()).hexdigest())
        elif isinstance(v, dict):
            for x in v.values():
                walk(x)
        elif isinstance(v, (tuple, list)):
            for x in v:
                walk(x)
    walk(w)
    return sorted(out)


def out_hash(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous().cpu()
        h.update(f"{t.dtype} {tuple(t.shape)} ".encode() + t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


class Recorder:
    """Recording wrappers on every entry point the binding knows, set on the library object; `restore()` puts the originals back."""

    def __init__(self):
        self.lib = _lib.load()
        self.lines = []
        self.orig = {n: getattr(self.lib, n) for n in _lib.HEADER.signatures}
        for n in self.orig:
            setattr(self.lib, n, self._wrap(n))

    def _wrap(self, name):
        fn = self.orig[name]

        def recording(*args):
            vals = []
            for a in args:
                s = getattr(a, "_obj", None)
                if isinstance(s, ctypes.Structure):
                    for f, t in s._fields_:
                        v = getattr(s, f)
                        vals.append(f"{f}={'set' if v else 'null'}" if issubclass(t, (ctypes.c_void_p, ctypes._Pointer)) else f"{f}={v!r}")
                elif isinstance(a, (int, float)) and not isinstance(a, bool):
                    vals.append(repr(a))
            self.lines.append(name + " " + " ".join(vals))
            return fn(*args)
        return recording

    def restore(self):
        for n, fn in self.orig.items():
            setattr(self.lib, n, fn)


def g(seed):
    return torch.Generator().manual_seed(seed)


def unet_case(cfg, seed, fused_ff=None):
    from evoworld_amd.unet import DEFAULT_CONFIG, UNetSpatioTemporalConditionModel, random_state_dict
    if fused_ff is not None:
        os.environ["EW_FUSED_FF"] = fused_ff
    try:
        fp8 = cfg.get("qkv_fp8", False)
        sd = random_state_dict({**DEFAULT_CONFIG, **{k: v for k, v in cfg.items() if k != "qkv_fp8"}}, seed)
        m = UNetSpatioTemporalConditionModel(**cfg).load_state_dict(sd, device=DEV)
    finally:
        os.environ.pop("EW_FUSED_FF", None)
    assert bool(m.fp8_blocks) == fp8
    B, T, h, w = 2, 4, 16, 32
    x = torch.randn(B, T, cfg["in_channels"], h, w, generator=g(1))
    ehs = torch.randn(B, 1, cfg["cross_attention_dim"], generator=g(2))
    ids = torch.tensor([[6.0, 127.0, 0.02]] * B)
    y = m(x.to(DEV), 500.0, ehs.to(DEV), ids.to(DEV), return_dict=False)[0]
    return m, (y,)


def vae_case():
    from evoworld_amd.vae import DEFAULT_VAE_CONFIG, AutoencoderKLTemporalDecoder, random_vae_state_dict
    from oracle.vae_ref import tiny_vae_config
    cfg = tiny_vae_config()
    sd = {k: v.half().float() for k, v in random_vae_state_dict({**DEFAULT_VAE_CONFIG, **cfg}, 0).items()}
    m = AutoencoderKLTemporalDecoder(**cfg).load_state_dict(sd, device=DEV)
    lat = m.encode((torch.rand(3, 3, 64, 128, generator=g(7)) * 2 - 1).to(DEV)).latent_dist.mode()
    z = torch.randn(4, 4, 8, 16, generator=g(8)).to(DEV)
    z6 = torch.randn(6, 4, 8, 16, generator=g(8)).to(DEV)
    return m, (lat, m.decode(z, num_frames=4).sample, m.decode(z6, num_frames=3).sample)


def clip_case():
    from evoworld_amd.clip import DEFAULT_CLIP_CONFIG, CLIPVisionModelWithProjection, random_clip_state_dict
    from oracle.clip_ref import tiny_clip_config
    cfg = tiny_clip_config()
    sd = {k: v.half().float() for k, v in random_clip_state_dict({**DEFAULT_CLIP_CONFIG, **cfg}, 0).items()}
    m = CLIPVisionModelWithProjection(**cfg).load_state_dict(sd, device=DEV)
    r = m(torch.randn(2, 3, 56, 56, generator=g(6)).to(DEV))
    return m, (r.image_embeds, r.last_hidden_state)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the document to this file")
    ap.add_argument("--detail-dir", help="write each case's launch trace as <case>.txt and its per-tensor hashes as <case>.weights.txt here (for reading a difference)")
    args = ap.parse_args()
    from oracle.unet_ref import tiny_config
    small = dict(tiny_config(), block_out_channels=(320, 128, 256, 256), num_attention_heads=(5, 2, 4, 4))
    cases = [("unet320_fused_ff", lambda: unet_case(small, 11, "1")),
             ("unet320_unfused_ff", lambda: unet_case(small, 11, "0")),
             ("unet_tiny_qkv_fp8", lambda: unet_case(dict(tiny_config(), qkv_fp8=True), 0)),
             ("vae_tiny", vae_case), ("clip_tiny", clip_case)]
    doc = {}
    for name, run in cases:
        rec = Recorder()
        try:
            with torch.no_grad():
                model, outs = run()
            torch.cuda.synchronize()
        finally:
            rec.restore()
        text = "\n".join(rec.lines) + "\n"
        hashes = "\n".join(tensor_hashes(model.w)) + "\n"
        doc[name] = {"weights": {"tensors": hashes.count("\n"), "sha256": hashlib.sha256(hashes.encode()).hexdigest()}, "launches": len(rec.lines),
                     "trace": hashlib.sha256(text.encode()).hexdigest(), "output": out_hash(*outs)}
        if args.detail_dir:
            os.makedirs(args.detail_dir, exist_ok=True)
            for fn, body in ((name + ".txt", text), (name + ".weights.txt", hashes)):
                with open(os.path.join(args.detail_dir, fn), "w") as f:
                    f.write(body)
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
