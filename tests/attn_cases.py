"""Cases and checks shared by the attention tests (a plain module, imported like glue_cases / ff_cases; CPU tensors only).

- one-hot cases: keys in {-1, +1}^D, query i = a * key pi(i).  The matching key's exponent exceeds every other key's by >= MIN_MARGIN
  log2 units (margin_log2 measures it, the CPU test asserts it), so that in every kernel P is exactly 1 for pi(i) and exactly 0
  elsewhere and the output row IS v[pi(i)], bit for bit.  check_gather compares the bits and, on a mismatch, looks the received row up
  among all V rows of the call: "query (seq, head, i) received the row of key (seq', head', j'), expected j" or "no V row".
- attn_tiled: torch restatement of the kernels' NUMERICS (fp32 scores rounded once per MFMA k-step of 16 channels, keys in tiles, P rounded to fp16, the normaliser summed from the
  same rounded values, fp32 rescale) under the three running-max policies: `exact` (temporal kernels), `deferred` (ew_attn_spatial_f16:
  raise when a tile exceeds the running max by 2^6) and `lazy` (ew_attn_spatial_log2_f16: look at the max on the first tile, afterwards
  only when a lane's row sum of a tile exceeds 2^10).  `fp32` is ew_attn_small_f16 (no tiles, no fp16 P).
- layouts: problems [P, S, D] <-> the token-major rows the entry points take (spatial: qk rows + V^T; temporal / small: q|k|v rows).
- profiles: the adversarial score profiles (shift, the seven lazy-max patterns, spike_case), in log2 units, with to_form() converting
  them to either spatial kernel's operands.
tests/test_cpu_attn_cases.py shows on the CPU that each check catches what it claims."""
import math

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
QK_LOG2_PRESCALE = (0.125 * LOG2E) ** 0.5      # == evoworld_amd.ops.QK_LOG2_PRESCALE (head_dim 64)
# match - max(other) in log2 units that every one-hot case must have: 25 bits take P below half of fp16's smallest denormal, 10 more cover the
# log2 form's lazy max (a tile is accumulated up to 2^10 above the running max before the max is looked at), the rest is spare
MIN_MARGIN = 40.0
DEFER_THR, SUM_CHECK_THR, SUM_RAISE_THR = 6.0, 1024.0, 4.0      # attention.hip


# ----------------------------------------------------------------------------- one-hot cases
def permutation(kind, S):
    """`affine`: pi(i) = (m i + 5) mod S, m the smallest odd number >= max(3, 3S/8) coprime to S (consecutive queries jump across
    the key tiles: queries of the last q-tile have targets in the first key tile and the reverse); `reverse`: pi(i) = S-1-i (key S-1,
    the last valid key of a ragged tile, belongs to query 0; keys 63 / 64 are hit)."""
    i = torch.arange(S)
    if kind == "reverse":
        return S - 1 - i
    assert kind == "affine", kind
    m = next(m for m in range(max(3, 3 * S // 8) | 1, 4 * S + 8, 2) if math.gcd(m, S) == 1)
    pi = (m * i + 5) % S
    assert pi.unique().numel() == S
    return pi


def _values(n, D, g):
    """random fp16, nonzero: random sign and mantissa, magnitude in [0.25, 4) -- the bounded range is part of the exactness argument:
    what was accumulated before the target arrives is rescaled to <= 2^-MIN_MARGIN * S * 16 * |v|, far below half an fp16 ulp"""
    bits = torch.randint(0, 1 << 10, (n, D), generator=g) | (torch.randint(13, 17, (n, D), generator=g) << 10)
    bits = bits | (torch.randint(0, 2, (n, D), generator=g) << 15)
    return (bits - ((bits >> 15) << 16)).to(torch.int16).view(torch.float16)


def onehot_call(ids, S, D, a, perm, seed=0):
    """One call's worth of one-hot problems.  ids: one tuple per problem, e.g. (seq, head) or (b, pixel, head) in the kernel's problem
    order.  Returns dict(q, k, v fp16 [P, S, D], target int64 [P, S], ids, S, D); every problem is drawn from its own seed."""
    assert a > 0 and math.log2(a) == int(math.log2(a)), "a must be a power of two: q = a * k stays exact"
    P = len(ids)
    k = torch.empty(P, S, D)
    v = torch.empty(P, S, D, dtype=torch.float16)
    target = torch.empty(P, S, dtype=torch.int64)
    for p in range(P):
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * p + S)
        k[p] = torch.randint(0, 2, (S, D), generator=g).float() * 2 - 1
        v[p] = _values(S, D, g)
        target[p] = permutation(perm, S)
    q = a * torch.gather(k, 1, target[:, :, None].expand(P, S, D))
    vi = v.view(torch.int16).reshape(P * S, D)
    assert bool(((vi & 0x7FFF) != 0).all()), "a zero value"
    assert torch.unique(vi, dim=0).shape[0] == P * S, "two equal V rows in one call: the lookup could not tell them apart"
    return dict(q=q.half(), k=k.half(), v=v, target=target, ids=list(ids), S=S, D=D)


def margin_log2(case, c):
    """min over all queries of (score of the target - largest other score) * c; c = log2 units per score unit (scale * log2 e, or 1 for
    the log2 form).  The scores are small integers times a: exact."""
    s = case["q"].double() @ case["k"].double().transpose(1, 2)                 # [P, S(query), S(key)]
    t = case["target"][:, :, None]
    match = torch.gather(s, 2, t)
    other = s.scatter(2, t, -math.inf).amax(dim=2, keepdim=True) if case["S"] > 1 else match - math.inf
    return float(((match - other) * c).min())


def expected_gather(case):
    P, S, D = case["v"].shape
    return torch.gather(case["v"], 1, case["target"][:, :, None].expand(P, S, D))


def check_gather(got, case, what="attention"):
    """got: fp16 [P, S, D] (any device).  Bit-exact against v[target]; the message names, for the first mismatching queries, which
    key's V row arrived instead."""
    got = got.detach().cpu().contiguous()
    exp = expected_gather(case)
    assert got.shape == exp.shape and got.dtype == torch.float16, (got.shape, got.dtype)
    gi, ei = got.view(torch.int16), exp.view(torch.int16)
    bad = (gi != ei).any(dim=2)
    if not bool(bad.any()):
        return
    P, S, D = exp.shape
    rows = {bytes(r.numpy().tobytes()): n for n, r in enumerate(case["v"].view(torch.int16).reshape(P * S, D))}
    lines = []
    for p, i in bad.nonzero().tolist()[:8]:
        n = rows.get(gi[p, i].numpy().tobytes())
        j = int(case["target"][p, i])
        if n is None:
            nd = int((gi[p, i] != ei[p, i]).sum())
            lines.append(f"query {(*case['ids'][p], i)} received no V row, expected key {j} ({nd} of {D} elements differ, "
                         f"first {got[p, i, :4].tolist()} vs {exp[p, i, :4].tolist()})")
        else:
            lines.append(f"query {(*case['ids'][p], i)} received the row of key {(*case['ids'][n // S], n % S)}, expected {j}")
    raise AssertionError(f"{what}: {int(bad.sum())} of {P * S} queries did not receive their key's V row bit for bit\n  " + "\n  ".join(lines))


# ----------------------------------------------------------------------------- the kernels' numerics
def _half_rtz(x):
    """fp32 >= 0 -> fp16 rounded toward zero (v_cvt_pkrtz_f16_f32: an overflow gives the largest finite value)"""
    x = x.clamp(max=65504.0)
    h = x.half()
    return (h.view(torch.int16) - (h.float() > x).to(torch.int16)).view(torch.float16)


def attn_tiled(q, k, v, c, policy, block=64, rtz=None):
    """q, k, v: fp16 [..., S, D] -> fp16 [..., S, D]; c: log2 units per score unit.  policy: `exact` | `deferred` | `lazy` | `fp32`
    (module docstring).  rtz: P rounded toward zero (the spatial kernels; default) or to nearest (the temporal ones).  More keys than
    queries are allowed (the emulated faults of the CPU test append some)."""
    S, Sk = q.shape[-2], k.shape[-2]
    qf, kf, vf = q.float(), k.float(), v.float()
    lead = q.shape[:-1]
    if policy == "fp32":                                                        # ew_attn_small_f16
        s = (qf * torch.tensor(c / LOG2E, dtype=torch.float32)) @ kf.transpose(-1, -2)
        p = torch.exp(s - s.amax(dim=-1, keepdim=True))
        return ((p @ vf) / p.sum(dim=-1, keepdim=True)).half()
    rtz = policy != "exact" if rtz is None else rtz
    rnd = _half_rtz if rtz else (lambda x: x.half())
    m = torch.zeros(lead) if policy == "lazy" else torch.full(lead, -math.inf)
    l = torch.zeros(lead)
    acc = torch.zeros(q.shape)
    half = (torch.arange(block) % 8) >= 4                                        # the keys of a tile that lane half lh = 1 holds
    qd, kd = q.double(), k.double()

    def mfma_scores(k0, init):
        """the score MFMAs: four k-steps of 16 channels, each an exact product sum added to the fp32 accumulator (one rounding per step)"""
        s = init[..., None].expand(*lead, min(block, Sk - k0)).float()
        for d0 in range(0, q.shape[-1], 16):
            s = (s.double() + qd[..., d0:d0 + 16] @ kd[..., k0:k0 + block, d0:d0 + 16].transpose(-1, -2)).float()
        return s

    for k0 in range(0, Sk, block):                                              # keys >= S do not exist here
        hb = half[: min(block, Sk - k0)]
        if policy == "lazy":
            s = mfma_scores(k0, -m)                                             # the C operand subtracts the running max
            tmax = s.amax(dim=-1)
            delta = tmax if k0 == 0 else torch.zeros(lead)                      # the first tile sets the max whatever its sign
            p = rnd(torch.exp2(s - delta[..., None]))
            if k0:
                over = ~((p[..., ~hb].float().sum(-1) <= SUM_CHECK_THR) & (p[..., hb].float().sum(-1) <= SUM_CHECK_THR))
                pad = (-S) % 32                                                 # the check is one vote per wave of 32 queries
                wave = F.pad(over, (0, pad)).reshape(*over.shape[:-1], -1, 32).any(dim=-1)
                trip = wave[..., None].expand(*wave.shape, 32).reshape(*over.shape[:-1], -1)[..., :S]
                delta = torch.where(trip & (tmax > SUM_RAISE_THR), tmax, delta)
                p = torch.where(trip[..., None], rnd(torch.exp2(s - delta[..., None])), p)
            m_new = m + delta
        else:
            s = mfma_scores(k0, torch.zeros(lead))
            mt = s.amax(dim=-1) * torch.tensor(c, dtype=torch.float32)
            m_new = torch.where(mt > m + DEFER_THR, mt, m) if policy == "deferred" else torch.maximum(m, mt)
            p = rnd(torch.exp2((s.double() * float(torch.tensor(c, dtype=torch.float32)) - m_new.double()[..., None]).float()))   # one rounding: an fma
        alpha = torch.exp2(m - m_new) if not (policy == "lazy" and k0 == 0) else torch.ones(lead)
        l = l * alpha + p.float().sum(dim=-1)
        acc = acc * alpha[..., None] + p.float() @ vf[..., k0:k0 + block, :]
        m = m_new
    return (acc * (1.0 / l)[..., None]).half()


def sdpa64(q, k, v, c):
    """fp64 softmax_2(c q k^T) v of fp16 [..., S, D] operands: the reference of every tolerance test"""
    return F.scaled_dot_product_attention(q.double(), k.double(), v.double(), scale=c / LOG2E)


# ----------------------------------------------------------------------------- layouts
def spatial_rows(x, n_seq, S, heads):
    """[P = n_seq*heads, S, 64] in (seq, head) order -> token-major rows [n_seq*S, heads*64]"""
    return x.reshape(n_seq, heads, S, 64).permute(0, 2, 1, 3).reshape(n_seq * S, heads * 64)


def spatial_problems(rows, n_seq, S, heads):
    return rows.reshape(n_seq, S, heads, 64).permute(0, 2, 1, 3).reshape(n_seq * heads, S, 64)


def temporal_rows(x, B, T, S, heads):
    """[P = B*S*heads, T, 64] in (b, pixel, head) order -> rows [(b*T + t)*S + pixel, heads*64]"""
    return x.reshape(B, S, heads, T, 64).permute(0, 3, 1, 2, 4).reshape(B * T * S, heads * 64)


def temporal_problems(rows, B, T, S, heads):
    return rows.reshape(B, T, S, heads, 64).permute(0, 2, 3, 1, 4).reshape(B * S * heads, T, 64)


def small_rows(x, n_seq, S, heads, D):
    return x.reshape(n_seq, heads, S, D).permute(0, 2, 1, 3).reshape(n_seq * S, heads * D)


def small_problems(rows, n_seq, S, heads, D):
    return rows.reshape(n_seq, S, heads, D).permute(0, 2, 1, 3).reshape(n_seq * heads, S, D)


def spatial_ids(n_seq, heads):
    return [(s, h) for s in range(n_seq) for h in range(heads)]


def temporal_ids(B, S, heads):
    return [(b, s, h) for b in range(B) for s in range(S) for h in range(heads)]


# ----------------------------------------------------------------------------- random operands and score profiles (log2 units)
def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def to_form(qk_l2, form):
    """fp32 q|k in log2 units (q.k IS the exponent) -> (fp16 operands, scale argument, c) of ew_attn_spatial_log2_f16 (`log2`: as they
    are) or ew_attn_spatial_f16 (`scale`: divided by sqrt(0.125 log2 e) each, so that q.k * 0.125 * log2 e is the same exponent)"""
    if form == "log2":
        return qk_l2.half(), None, 1.0
    assert form == "scale", form
    return (qk_l2 / QK_LOG2_PRESCALE).half(), 0.125, 0.125 * LOG2E


def spatial_random(n_seq, S, heads):
    """the operands of test_attn_spatial: q|k fp32 [rows, 2C] in natural units (x QK_LOG2_PRESCALE: log2 units), v fp16 [rows, C]"""
    C, rows = heads * 64, n_seq * S
    qk32 = _rnd(rows, 2 * C, seed=1)
    qk32[: S // 2, :64] *= 4.0                      # sharpen some rows so the running max moves between tiles
    return qk32, _rnd(rows, C, seed=2).half()


def shift_case(n_seq, S, heads, shift):
    """`shift` moves every score of a head by a constant (one extra q / k channel pair): strongly negative first-tile maxima (the max
    must be SET on the first tile, not only raised) and large positive ones (raises).  -> q|k fp32 in log2 units, v fp16"""
    C = heads * 64
    qk32, v = spatial_random(n_seq, S, heads)
    if shift:
        qk32[:, 0] = abs(shift) ** 0.5 * 8 ** 0.5  # q_0 * k_0 * scale = shift
        qk32[:, C] = (1 if shift > 0 else -1) * abs(shift) ** 0.5 * 8 ** 0.5
        qk32[S // 3:, C] *= 0.5                    # ... and smaller for later keys: the first tile holds the max
    return qk32 * QK_LOG2_PRESCALE, v


SHIFT_CASES = [(2, 512, 2, 0.0), (1, 1000, 1, 0.0), (3, 136, 5, 0.0), (1, 2304, 1, -60.0), (1, 640, 2, 40.0), (1, 128, 1, -60.0),
               (2, 72, 2, 40.0)]
LAZY_PATTERNS = ["ramp", "jumps", "overflow", "flat_below", "flat_above", "late_spike", "ragged_spike"]
# plateaus just below / just above the decision of each form: the log2 form's row-sum limit (32 keys x 2^4.9 = 955 < 1024 < 32 x 2^5.1) and the
# scale form's deferred raise (a tile maximum 5.9 / 6.1 above the running one, threshold 6)
PLATEAUS = {"log2": (4.9, 5.1), "scale": (5.9, 6.1)}


def lazy_max_case(pattern, form="log2"):
    """Score profiles that stress the decision when to look at / raise the running max: key j carries an offset f(j) in log2 units
    (q channel 0 = 1, k channel 0 = f) on top of random scores -- slow ramps (many small raises), jumps up and down, jumps large enough
    to overflow the exponentials before the check sees them, plateaus just below / just above the form's threshold, a spike in the very
    last (ragged) tile.  The second head sees the mirrored (falling) profile.  -> (n_seq, S, heads, q|k fp32 in log2 units, v fp16)"""
    n_seq, heads = 2, 2
    S = 1000 if pattern == "ragged_spike" else 1024
    C, rows = heads * 64, n_seq * S
    qk32 = _rnd(rows, 2 * C, seed=5) * 0.6
    v = _rnd(rows, C, seed=6).half()
    t = (torch.arange(S) // 64).float()
    lo, hi = PLATEAUS[form]
    f = {"ramp": 0.37 * t, "jumps": 30.0 * ((t % 3) == 2).float() - 12.0 * ((t % 5) == 1).float(), "overflow": 200.0 * t,
         "flat_below": lo * (t > 0).float(), "flat_above": hi * (t > 0).float(), "late_spike": 25.0 * (t == 15).float(),
         "ragged_spike": 40.0 * (torch.arange(S) >= 990).float()}[pattern]
    for h in range(heads):
        qk32[:, h * 64] = 1.0
        qk32[:, C + h * 64] = f.repeat(n_seq) * (1.0 if h == 0 else -0.5)
    return n_seq, S, heads, qk32, v


def spike_case(pattern, B=1, T=97, S=6, heads=1, seed=3):
    """fp16 q, k, v [B, T, S, heads, 64] that force the rescale: every query gets +16 u (u a unit vector); `first`: only key 3 gets +16 u (the
    maximum is set in the first block and never displaced); `last`: only key T-1 (the maximum jumps by ~40 logits in the final, one-key block of
    T = 97); `rising`: key t gets +(16 t / (T-1)) u (the maximum rises in every block)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, T, S, heads, 64, generator=g) for _ in range(3))
    u = torch.randn(64, generator=g)
    u = u / u.norm()
    q = q + 16.0 * u
    if pattern == "first":
        k[:, 3] += 16.0 * u
    elif pattern == "last":
        k[:, T - 1] += 16.0 * u
    elif pattern == "rising":
        k = k + (16.0 * torch.arange(T, dtype=torch.float32) / (T - 1))[None, :, None, None, None] * u
    else:
        raise ValueError(pattern)
    return q.half(), k.half(), v.half()


# ----------------------------------------------------------------------------- the one-hot cases of each kernel family
# (n_seq, S, heads): every S of {8, 72, 136, 200, 1000}, every n_seq and heads of {1, 2, 3}; 3x136x3 and 2x200x2 have both > 1
ONEHOT_SPATIAL = [(2, 8, 1), (1, 72, 3), (3, 136, 3), (2, 200, 2), (1, 1000, 2), (3, 8, 2)]
# (B, T, S pixels, heads): T covers the three kernels (<= 32, <= 64, streaming) at and beside their block edges; S*heads*B % 4 != 0: an idle wave
ONEHOT_TEMPORAL = [(1, 2, 5, 1), (2, 25, 7, 1), (1, 32, 5, 3), (1, 33, 7, 2), (2, 49, 5, 1), (1, 64, 7, 3), (1, 65, 5, 2), (1, 97, 7, 1),
                   (1, 129, 5, 3)]
ONEHOT_SMALL = [(2, 17, 3, 80), (1, 257, 2, 80), (2, 64, 2, 64)]              # (n_seq, S, heads, D)
PERMS = ["affine", "reverse"]
A_LOG2, A_SCALE = 2.0, 16.0         # q = a * k: log2 form 128 log2 units for the match; scale forms 16 * D * D^-0.5 * log2 e


def onehot_spatial(n_seq, S, heads, perm, form):
    case = onehot_call(spatial_ids(n_seq, heads), S, 64, A_LOG2 if form == "log2" else A_SCALE, perm, seed=1 + (form == "log2"))
    return case, (1.0 if form == "log2" else 0.125 * LOG2E)


def onehot_temporal(B, T, S, heads, perm):
    return onehot_call(temporal_ids(B, S, heads), T, 64, A_SCALE, perm, seed=3), 0.125 * LOG2E


def onehot_small(n_seq, S, heads, D, perm):
    return onehot_call(spatial_ids(n_seq, heads), S, D, A_SCALE, perm, seed=4), D ** -0.5 * LOG2E


def all_onehot_cases():
    """(name, case, c, policy, block) of every one-hot case of the GPU tests: the CPU test asserts the margin of each"""
    for n_seq, S, heads in ONEHOT_SPATIAL:
        for perm in PERMS:
            for form in ("scale", "log2"):
                case, c = onehot_spatial(n_seq, S, heads, perm, form)
                yield f"spatial_{form} {n_seq}x{S}x{heads} {perm}", case, c, "lazy" if form == "log2" else "deferred", 64
    for B, T, S, heads in ONEHOT_TEMPORAL:
        for perm in PERMS:
            case, c = onehot_temporal(B, T, S, heads, perm)
            yield f"temporal {B}x{T}x{S}x{heads} {perm}", case, c, "exact", 32 if T > 64 else 64
    for n_seq, S, heads, D in ONEHOT_SMALL:
        for perm in PERMS:
            case, c = onehot_small(n_seq, S, heads, D, perm)
            yield f"small {n_seq}x{S}x{heads}x{D} {perm}", case, c, "fp32", S
