"""The attention cases and checks of tests/attn_cases.py do what they claim (CPU only: the "kernels" are attn_tiled, the torch
restatement of the kernels' numerics, and emulated faults built on it)."""
import pytest
import torch

import attn_cases as ac
from attn_stream_ref import attn_stream
from kernel_checks import worst_row


@pytest.fixture(scope="module")
def onehot():
    return list(ac.all_onehot_cases())


def test_onehot_cases_cover_the_stated_shapes():
    assert {s for _, s, _ in ac.ONEHOT_SPATIAL} == {8, 72, 136, 200, 1000}
    assert {n for n, _, _ in ac.ONEHOT_SPATIAL} == {h for _, _, h in ac.ONEHOT_SPATIAL} == {1, 2, 3}
    assert any(n > 1 and h > 1 for n, _, h in ac.ONEHOT_SPATIAL)
    assert {t for _, t, _, _ in ac.ONEHOT_TEMPORAL} == {2, 25, 32, 33, 49, 64, 65, 97, 129}
    assert {s for _, _, s, _ in ac.ONEHOT_TEMPORAL} == {5, 7} and {b for b, _, _, _ in ac.ONEHOT_TEMPORAL} == {1, 2}
    assert all(h <= 3 for _, _, _, h in ac.ONEHOT_TEMPORAL) and any(b * s * h % 4 for b, _, s, h in ac.ONEHOT_TEMPORAL)   # an idle wave
    assert {(s, d) for _, s, _, d in ac.ONEHOT_SMALL} == {(17, 80), (257, 80), (64, 64)}


def test_permutations():
    for S in (2, 8, 25, 72, 136, 200, 1000):
        for kind in ac.PERMS:
            assert sorted(ac.permutation(kind, S).tolist()) == list(range(S))
    rev = ac.permutation("reverse", 136)
    assert rev[0] == 135 and rev[72] == 63 and rev[71] == 64            # the last key of the ragged tile; keys 63 / 64
    aff = ac.permutation("affine", 1000)
    assert (aff[896:] < 64).any() and (aff[:128] >= 960).any()          # last q-tile -> first key tile, first q-tile -> last key tile


def test_onehot_margin_is_at_least_40_log2_units(onehot):
    """the condition of the exact tests, for every query of every case: not a measurement, a requirement on the builder"""
    worst = {}
    for name, case, c, _, _ in onehot:
        mg = ac.margin_log2(case, c)
        fam = name.split()[0]
        worst[fam] = min(worst.get(fam, 1e9), mg)
        assert mg >= ac.MIN_MARGIN, (name, mg)
    print("smallest one-hot margins (log2 units):", {k: round(v, 1) for k, v in worst.items()})
    # a = 8 in the scale form is under the line at the larger sizes: why A_SCALE is 16
    low = ac.onehot_call(ac.spatial_ids(1, 1), 1000, 64, 8.0, "affine", seed=1)
    assert ac.margin_log2(low, 0.125 * ac.LOG2E) < 46


def test_onehot_values_are_nonzero_and_distinct():
    case = ac.onehot_call(ac.spatial_ids(2, 2), 72, 64, 16.0, "affine")
    v = case["v"]
    assert bool((v != 0).all()) and bool(torch.isfinite(v).all()) and 0.25 <= float(v.abs().min()) and float(v.abs().max()) < 4.0
    assert torch.unique(v.view(torch.int16).reshape(-1, 64), dim=0).shape[0] == 4 * 72
    assert not torch.equal(case["k"][0], case["k"][1])                  # every problem from its own seed
    assert torch.equal(case["q"], 16.0 * torch.gather(case["k"], 1, case["target"][:, :, None].expand(-1, -1, 64)))


def test_kernel_numerics_reproduce_the_gather_exactly(onehot):
    """fp32 scores, P rounded to fp16 (toward zero in the spatial forms), l summed from the rounded P, fp32 rescale: the output row is
    v[pi(i)] bit for bit under every running-max policy -- also where the target arrives in a later tile, after other keys were
    accumulated under a lower running max and rescaled"""
    late = 0
    for name, case, c, policy, block in onehot:
        got = ac.attn_tiled(case["q"], case["k"], case["v"], c, policy, block)
        ac.check_gather(got, case, name)
        late += int((case["target"] >= block).sum())
    assert late > 1000
    case, c = ac.onehot_temporal(1, 129, 5, 3, "affine")
    ac.check_gather(attn_stream(case["q"], case["k"], case["v"]), case, "attn_stream")


def test_gather_check_is_not_blind_to_one_bit():
    case, c = ac.onehot_spatial(2, 72, 1, "affine", "scale")
    got = ac.expected_gather(case).clone()
    ac.check_gather(got, case)
    got.view(torch.int16)[1, 40, 63] ^= 1
    with pytest.raises(AssertionError, match=r"query \(1, 0, 40\) received no V row, expected key"):
        ac.check_gather(got, case)


def test_lookup_names_two_keys_swapped_inside_a_16_key_group():
    """the V^T tile written in another order than the S^T accumulator yields: keys 4 and 8 of every 16 exchange their V rows"""
    case, c = ac.onehot_spatial(2, 136, 3, "reverse", "log2")
    j = torch.arange(136)
    full = j < 128                                                        # the eight whole groups
    swap = torch.where(full & (j % 16 == 4), j + 4, torch.where(full & (j % 16 == 8), j - 4, j))
    got = ac.attn_tiled(case["q"], case["k"], case["v"][:, swap], c, "lazy")
    with pytest.raises(AssertionError) as e:
        ac.check_gather(got, case)
    msg = str(e.value)
    # pi(i) = 135 - i: query 15 wants key 120 = 16*7 + 8 and query 19 key 116 = 16*7 + 4
    assert "query (0, 0, 15) received the row of key (0, 0, 116), expected 120" in msg
    assert "query (0, 0, 19) received the row of key (0, 0, 120), expected 116" in msg
    assert f"{2 * 3 * 2 * 8} of {6 * 136} queries" in msg


def test_lookup_names_a_tail_key_admitted():
    """mask_tail one key short: key S of the ragged tile (its K row clamped to S-1, its V^T column zero) reaches the softmax -- the
    query whose target is S-1 sees two equal maxima, l = 2, and gets half of v[S-1]: no V row"""
    case, c = ac.onehot_spatial(1, 72, 3, "reverse", "scale")
    k = torch.cat([case["k"], case["k"][:, -1:]], dim=1)
    v = torch.cat([case["v"], torch.zeros(3, 1, 64, dtype=torch.float16)], dim=1)
    got = ac.attn_tiled(case["q"], k, v, c, "deferred")
    with pytest.raises(AssertionError) as e:
        ac.check_gather(got, case)
    msg = str(e.value)
    assert "3 of 216 queries" in msg
    for h in range(3):
        assert f"query (0, {h}, 0) received no V row, expected key 71 (64 of 64 elements differ" in msg


def test_lookup_names_the_neighbouring_sequence():
    """tok0 one sequence off in the V^T address: every query receives the right key's row of the wrong sequence"""
    B, T, S, heads = 2, 25, 7, 1
    case, c = ac.onehot_temporal(B, T, S, heads, "affine")
    got = ac.attn_tiled(case["q"], case["k"], case["v"].roll(-1, dims=0), c, "exact")
    with pytest.raises(AssertionError) as e:
        ac.check_gather(got, case)
    msg = str(e.value)
    t0 = int(case["target"][0, 0])
    assert f"query (0, 0, 0, 0) received the row of key (0, 1, 0, {t0}), expected {t0}" in msg
    assert f"{B * S * T} of {B * S * T} queries" in msg


def test_layouts_round_trip_and_place_heads():
    x = torch.arange(6 * 8 * 64, dtype=torch.float32).reshape(6, 8, 64)
    rows = ac.spatial_rows(x, 2, 8, 3)
    assert torch.equal(ac.spatial_problems(rows, 2, 8, 3), x)
    assert torch.equal(rows[1 * 8 + 5, 2 * 64:3 * 64], x[1 * 3 + 2, 5])                 # (seq 1, head 2), token 5
    y = torch.arange(2 * 5 * 3 * 4 * 64, dtype=torch.float32).reshape(30, 4, 64)
    rows = ac.temporal_rows(y, 2, 4, 5, 3)
    assert torch.equal(ac.temporal_problems(rows, 2, 4, 5, 3), y)
    assert torch.equal(rows[(1 * 4 + 2) * 5 + 3, 64:128], y[(1 * 5 + 3) * 3 + 1, 2])      # b 1, frame 2, pixel 3, head 1
    z = torch.arange(4 * 17 * 80, dtype=torch.float32).reshape(4, 17, 80)
    assert torch.equal(ac.small_problems(ac.small_rows(z, 2, 17, 2, 80), 2, 17, 2, 80), z)
    assert ac.spatial_ids(2, 2) == [(0, 0), (0, 1), (1, 0), (1, 1)] and ac.temporal_ids(1, 2, 2) == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1)]


def _spatial_emulation_worst_row(qk_l2, v, n_seq, S, heads, form):
    qk, _, c = ac.to_form(qk_l2, form)
    C = heads * 64
    q, k, vv = (ac.spatial_problems(x, n_seq, S, heads) for x in (qk[:, :C], qk[:, C:], v))
    got = ac.attn_tiled(q, k, vv, c, "lazy" if form == "log2" else "deferred")
    assert torch.isfinite(got).all()
    return worst_row(ac.spatial_rows(got, n_seq, S, heads), ac.spatial_rows(ac.sdpa64(q, k, vv, c), n_seq, S, heads))[0]


@pytest.mark.parametrize("form", ["log2", "scale"])
def test_fp16_p_algorithm_stays_under_the_per_row_ceiling_on_every_profile(form):
    """the 1e-3 per-row ceiling of the GPU tests is reachable by the algorithm itself (fp16 P, rounded-sum normaliser) on every profile"""
    out = {}
    for pattern in ac.LAZY_PATTERNS:
        n_seq, S, heads, qk_l2, v = ac.lazy_max_case(pattern, form)
        out[pattern] = _spatial_emulation_worst_row(qk_l2, v, n_seq, S, heads, form)
    for n_seq, S, heads, shift in ac.SHIFT_CASES:
        out[f"shift {n_seq}x{S}x{heads} {shift}"] = _spatial_emulation_worst_row(*ac.shift_case(n_seq, S, heads, shift), n_seq, S, heads, form)
    print(f"worst rows of the {form} emulation:", {k: f"{v:.2e}" for k, v in out.items()})
    assert max(out.values()) < 1e-3, out


@pytest.mark.parametrize("T", [25, 49, 97])
@pytest.mark.parametrize("pattern", ["first", "last", "rising"])
def test_fp16_p_algorithm_under_the_ceiling_on_the_spikes(pattern, T):
    q, k, v = ac.spike_case(pattern, T=T)
    B, _, S, heads, _ = q.shape
    p = lambda x: ac.temporal_problems(x.reshape(B * T * S, heads * 64), B, T, S, heads)
    got = ac.attn_tiled(p(q), p(k), p(v), 0.125 * ac.LOG2E, "exact", 32 if T > 64 else 64)
    w = worst_row(ac.temporal_rows(got, B, T, S, heads), ac.temporal_rows(ac.sdpa64(p(q), p(k), p(v), 0.125 * ac.LOG2E), B, T, S, heads))[0]
    print(f"spike {pattern} T={T}: worst row {w:.2e}")
    assert w < 1e-3


def test_profiles_hit_both_sides_of_each_decision():
    """flat_below / flat_above are aimed at each form's threshold: the log2 form's row-sum limit and the scale form's deferred raise"""
    assert 32 * 2 ** ac.PLATEAUS["log2"][0] < ac.SUM_CHECK_THR < 32 * 2 ** ac.PLATEAUS["log2"][1]
    assert ac.PLATEAUS["scale"][0] < ac.DEFER_THR < ac.PLATEAUS["scale"][1]
    n_seq, S, heads, qk_l2, v = ac.lazy_max_case("flat_above", "scale")
    qk, scale, c = ac.to_form(qk_l2, "scale")
    assert scale == 0.125 and abs(float(qk[0, 0]) * float(qk[100, 128]) * c - 6.1) < 0.02          # the offset survives the conversion
    ql, _, _ = ac.to_form(qk_l2, "log2")
    e_l = ql[:8, :64].double() @ ql[:70, 128:192].double().T
    e_s = (qk[:8, :64].double() @ qk[:70, 128:192].double().T) * c
    assert float((e_l - e_s).abs().max()) < 0.05                                                   # same exponents in both forms
