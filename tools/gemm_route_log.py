"""Routing log of ew_gemm_f16 on the product's own problems, for comparing two builds of the library (EW_LIB_PATH selects one).
Default: one full-size U-Net forward, VAE encode + decode and CLIP forward on seeded inputs under generation 3, generation 3 with
ew_set_gemm_debug(4), generation 2 and generation 1; one line per ops.gemm call (argument shape, kernel launched) and a SHA-256
of every final output.  --graph: three ops.gemm calls captured on a fresh stream that has no stream-K workspace, replayed once.
--host-time: host time per ops.gemm call (enqueue only, small problems) on the generation-3, generation-2 and generation-1 routes.
Two builds with identical device code must print identical logs: any difference is a routing or schedule difference."""
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from evoworld_amd import _lib, ops  # noqa: E402

lib = _lib.load()
_gemm = ops.gemm


def logged_gemm(a, w, out, **kw):
    r = _gemm(a, w, out, **kw)
    r1, r2 = kw.get("r1"), kw.get("r2")
    lo = [n for n, t in (("r1_lo", r1), ("r2_lo", r2), ("out_lo", out)) if isinstance(t, ops.Res) and t.lo is not None]
    opnds = [n for n in ("rowbias", "r1", "r2") if kw.get(n) is not None] + lo
    print(f"gemm mode={kw.get('mode', 0)} M={kw['M']} N={kw['N']} C={kw['c1'] + kw.get('c2', 0)} act={kw.get('act', 0)} "
          f"[{' '.join(opnds)}] -> {lib.ew_gemm_last_kernel().decode()}")
    return r


ops.gemm = logged_gemm


def sha(name, t):
    t = t.hi if isinstance(t, ops.Res) else t
    print(f"sha256 {name} {hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()}", flush=True)


def models():
    from evoworld_amd.clip import CLIPVisionModelWithProjection, encode_image_preprocess
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel
    from evoworld_amd.vae import AutoencoderKLTemporalDecoder
    unet = UNetSpatioTemporalConditionModel.from_random(seed=0, device="cuda")
    vae = AutoencoderKLTemporalDecoder.from_random(seed=0, device="cuda")
    clip = CLIPVisionModelWithProjection.from_random(seed=0, device="cuda")
    g = torch.Generator().manual_seed(0)
    sample = torch.randn(2, 25, unet._cfg["in_channels"], 72, 128, generator=g).cuda()
    ehs = torch.randn(2, 1, 1024, generator=g).cuda().half()
    added = torch.tensor([[6.0, 127.0, 0.02]] * 2, device="cuda")
    frames = (torch.rand(26, 3, 576, 1024, generator=g) * 2 - 1).cuda()
    lat = torch.randn(25, 4, 72, 128, generator=g).cuda()
    for gen, dbg in ((3, 0), (3, 4), (2, 0), (1, 0)):
        print(f"==== generation {gen} debug {dbg}", flush=True)
        lib.ew_set_gemm_generation(gen)
        lib.ew_set_gemm_debug(dbg)
        sha("unet", unet(sample, 1.234, ehs, added).sample)
        sha("vae_encode", vae.encode(frames).latent_dist.mode())
        sha("vae_decode", torch.cat([vae.decode(lat[i:i + 8], num_frames=min(8, 25 - i)).sample for i in range(0, 25, 8)]))
        sha("clip", clip(encode_image_preprocess(frames[:1] / 2 + 0.5)).image_embeds)
        print(f"ew_gemm_streamk_status {lib.ew_gemm_streamk_status()}", flush=True)


def graph():
    g = torch.Generator().manual_seed(0)
    cases = []       # (M, N, C, mode, conv): tail-split shape (1800 tiles), half-split shape (116 tiles, K = 11520), a plain dense GEMM
    for M, N, C, mode, conv in ((460800, 320, 320, ops.A_CONV3X3, (50, 72, 128, 72, 128, 1, 0)),
                                (7200, 1280, 1280, ops.A_CONV3X3, (50, 9, 16, 9, 16, 1, 0)), (7200, 1280, 1280, ops.A_DENSE, None)):
        taps = 9 if conv else 1
        a = (torch.randn(M, C, generator=g) * 0.5).cuda().half()
        w = (torch.randn(N, taps * C, generator=g) * 0.02).cuda().half()
        cases.append((a, w, torch.zeros(M, N, dtype=torch.float16, device="cuda"), dict(M=M, N=N, c1=C, lda=C, mode=mode, conv=conv)))
    ops.gemm = _gemm
    for gen in (2, 3):      # every kernel the capture can choose has run once on the default stream (its LDS attribute is set)
        lib.ew_set_gemm_generation(gen)
        lib.ew_set_gemm_debug(4)
        for a, w, out, kw in cases:
            ops.gemm(a, w, out, **kw)
    lib.ew_set_gemm_debug(0)
    torch.cuda.synchronize()
    ops.gemm = logged_gemm
    side, cg = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    print("==== capture on a fresh stream without ew_gemm_streamk_init", flush=True)
    with torch.cuda.graph(cg, stream=side):
        for a, w, out, kw in cases:
            ops.gemm(a, w, out, **kw)
    for _, _, out, _ in cases:
        out.zero_()
    torch.cuda.synchronize()
    cg.replay()
    torch.cuda.synchronize()
    for i, (_, _, out, _) in enumerate(cases):
        sha(f"graph_out{i}", out)
    print(f"ew_gemm_streamk_status {lib.ew_gemm_streamk_status()}", flush=True)


def host_time():
    ops.gemm = _gemm
    ops.streamk_init()
    for name, gen, M, N, conv, n in (("gen3 whole tiles", 3, 51200, 320, None, 4000), ("gen3 tail split", 3, 81920, 320, (10, 64, 128, 64, 128, 1, 0), 1000),
                                     ("gen2", 3, 1024, 320, None, 4000), ("gen1", 1, 1024, 320, None, 4000)):
        lib.ew_set_gemm_generation(gen)
        a = torch.randn(M, 64, device="cuda").half()
        w = torch.randn(N, (9 if conv else 1) * 64, device="cuda").half() * 0.02
        out = torch.zeros(M, N, dtype=torch.float16, device="cuda")
        kw = dict(M=M, N=N, c1=64, lda=64, mode=ops.A_CONV3X3 if conv else ops.A_DENSE, conv=conv)
        best = float("inf")
        for _ in range(6):                       # the first pass is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                ops.gemm(a, w, out, **kw)
            best = min(best, (time.perf_counter() - t0) / n * 1e6)
        torch.cuda.synchronize()
        print(f"{name:18s} {lib.ew_gemm_last_kernel().decode():40s} host us/call, best of 6 x {n}: {best:.2f}", flush=True)
    print(f"ew_gemm_streamk_status {lib.ew_gemm_streamk_status()}", flush=True)


with torch.no_grad():
    graph() if "--graph" in sys.argv else host_time() if "--host-time" in sys.argv else models()
