"""Stand-alone timing of ew_attn_spatial_f16 at the level-0 shape (250 problems x S=9216 x 64) for counter runs.
With --temporal T [T ...]: the temporal core (ew_attn_temporal_f16) at the level-0 shape instead (B = 2, S = 72*128, 5 heads, ld = 960, ld_o = 320;
env B, S) at each frame count T, any T > 0, on random data, in interleaved rounds: ms and GB/s of algorithmic bytes (q, k, v read once, o written
once)."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from evoworld_amd import ops


def temporal(frames):
    B, S, heads = int(os.environ.get("B", 2)), int(os.environ.get("S", 72 * 128)), 5
    C = heads * 64
    iters = int(os.environ.get("ITERS", 20))
    g = torch.Generator(device="cuda").manual_seed(0)
    bufs = {}
    for T in frames:
        rows = B * T * S
        bufs[T] = (torch.randn(rows, 3 * C, generator=g, device="cuda", dtype=torch.float16), torch.empty(rows, C, dtype=torch.float16, device="cuda"))
    for rep in range(int(os.environ.get("REPS", 3))):
        for T in frames:
            qkv, o = bufs[T]
            fn = lambda: ops.attn_temporal(qkv, qkv[:, C:], qkv[:, 2 * C:], o, B, T, S, heads, 3 * C, C)
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            ms = s.elapsed_time(e) / iters
            print(f"attn_temporal B={B} T={T} S={S} h={heads}: {ms:.3f} ms  {B * T * S * 4 * C * 2 / ms / 1e6:.0f} GB/s", flush=True)
        assert all(bool(torch.isfinite(bufs[T][1][:4096]).all()) for T in frames)


if len(sys.argv) > 1 and sys.argv[1] == "--temporal":
    temporal([int(a) for a in sys.argv[2:]] or [64, 97, 128])
    sys.exit(0)
n_seq, S, heads = int(os.environ.get("NSEQ", 50)), int(os.environ.get("S", 9216)), 5
C, rows = heads * 64, n_seq * S
g = torch.Generator().manual_seed(0)
qk = torch.randn(rows, 2 * C, generator=g).half().cuda()
vt = torch.randn(C, rows, generator=g).half().cuda()
o = torch.empty(rows, C, dtype=torch.float16, device="cuda")
iters = int(os.environ.get("ITERS", 3))
qk2 = (qk.float() * ops.QK_LOG2_PRESCALE).half()          # what the projection epilogue hands ew_attn_spatial_log2_f16
o2 = torch.empty_like(o)
fl = 4.0 * n_seq * heads * S * S * 64
for rep in range(int(os.environ.get("REPS", 2))):
    for name, fn in (("attn_spatial     ", lambda: ops.attn_spatial(qk, qk[:, C:], vt, o, n_seq, S, heads, 2 * C, rows, C)),
                     ("attn_spatial_log2", lambda: ops.attn_spatial_log2(qk2, qk2[:, C:], vt, o2, n_seq, S, heads, 2 * C, rows, C))):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / iters
        print(f"{name} n_seq={n_seq} S={S}: {ms:.3f} ms  {fl / ms / 1e9:.1f} TF/s", flush=True)
d = (o.float() - o2.float()).norm() / o.float().norm()
print(f"log2 form vs scale-and-shift form: rel-L2 {d:.2e}")
