"""-m 'not gpu': the non-curve navigation mode's segmentation (Navigator.split_path_into_segments) against the reference's own
split_path_into_segments (navigator_evoworld.py:276-301) on three paths, tests/golden/navigate_path.npz (a)."""
import numpy as np
import pytest
import torch


@pytest.mark.parametrize("tag", ["case000", "loop", "turns"])
def test_split_path_into_segments_matches_reference(golden_dir, tag):
    from evoworld_amd.inference import Navigator
    g = np.load(f"{golden_dir}/navigate_path.npz")
    path = torch.from_numpy(g[f"a_{tag}_path"].copy())
    segs = Navigator.split_path_into_segments(path)
    assert [len(s) for s in segs] == g[f"a_{tag}_lengths"].tolist()
    assert all(s.dtype == torch.float32 for s in segs)
    assert np.array_equal(torch.cat(segs).numpy(), g[f"a_{tag}_segments"])


@pytest.mark.parametrize("tag", ["case000", "turns"])
def test_split_path_leaves_the_callers_poses_alone(golden_dir, tag):
    """The reference writes into its input on consecutive turns (the golden records that); the build never does, and a second
    call on the same tensor gives the segments of the pristine poses, as the reference's fresh per-call copies do."""
    from evoworld_amd.inference import Navigator
    g = np.load(f"{golden_dir}/navigate_path.npz")
    pristine = g[f"a_{tag}_path"]
    assert not np.array_equal(g[f"a_{tag}_path_after"], pristine)
    path = torch.from_numpy(pristine.copy())
    first = Navigator.split_path_into_segments(path)
    assert np.array_equal(path.numpy(), pristine)
    again = Navigator.split_path_into_segments(path)
    assert len(again) == len(first) and all(torch.equal(a, b) for a, b in zip(first, again))


def test_split_path_turn_semantics():
    """A turn starts a segment with the previous position and the new rotation; allclose(atol=1e-5) also applies rtol=1e-5."""
    from evoworld_amd.inference import Navigator
    p = torch.tensor([[0.0, 0, 0.0, 0, 90.0, 0], [0.1, 0, 0.0, 0, 90.0, 0], [0.1, 0, 0.1, 0, 0.0, 0],
                      [0.1, 0, 0.2, 0, 0.0005, 0], [0.1, 0, 0.3, 0, 0.0005, 0]])
    segs = Navigator.split_path_into_segments(p)
    assert [len(s) for s in segs] == [2, 2, 3]
    assert segs[1][0].tolist() == [p[1, 0].item(), 0, 0, 0, 0, 0] and torch.equal(segs[1][1], p[2])
    q = torch.tensor([[0.0, 0, 0, 0, 1000.0, 0], [0.0, 0, 1, 0, 1000.005, 0]])      # |d| = 0.005 <= 1e-5 + 1e-5 * 1000
    assert [len(s) for s in Navigator.split_path_into_segments(q)] == [2]


def test_path_episode_check_refuses_single_frame_hand_offs(golden_dir):
    """A path that turns at every pose (the curve-mode synthetic episode, the reference's case_000) starts with a 1-pose run:
    segment 0 keeps one frame, and the memory hand-off cannot align on it -- refused with the segment named, before any work."""
    import unified_loop_consistency as cli
    from evoworld_amd.inference import Navigator, check_path_episode
    curvy = torch.tensor(cli.synthetic_episode(56), dtype=torch.float32)
    runs = [len(r) for r in Navigator.split_path_into_segments(curvy)]
    assert runs[:3] == [1, 2, 2]
    with pytest.raises(ValueError, match="segment 0: the memory hand-off would align on 1 generated frame"):
        check_path_episode(runs, 56, 2)
    case000 = np.load(f"{golden_dir}/navigate_path.npz")["a_case000_lengths"].tolist()
    with pytest.raises(ValueError, match="segment 0"):
        check_path_episode(case000, sum(case000), 3)
    check_path_episode(runs, 56, 1)                               # one segment: no hand-off
    check_path_episode([2, 2, 2], 73, 3)                          # 2 then 3 frames: enough to align
    check_path_episode([10, 61], 70, 2)                           # short first run: 10 frames reach the hand-off
    with pytest.raises(ValueError, match="segment 1: the memory for segment 2"):
        check_path_episode([10, 61, 5], 70, 3)
    with pytest.raises(ValueError, match="segment 2: the path splits into only 2"):
        check_path_episode([25, 49], 73, 3)


@pytest.mark.parametrize("num_segments", [1, 2, 3, 4])
def test_cli_synthetic_path_episode_is_runnable(num_segments):
    """Without --curve_path the CLI's synthetic episode is piecewise straight: runs of 25 poses after the split, 25 / 49 / 73 ...
    frames, enough poses for every hand-off."""
    import unified_loop_consistency as cli
    from evoworld_amd.inference import Navigator, check_path_episode
    cam = cli.synthetic_path_episode(num_segments)
    scaled = torch.tensor(cam, dtype=torch.float32)
    scaled[:, :3] *= 0.1
    runs = [len(r) for r in Navigator.split_path_into_segments(scaled)]
    assert runs == [25] * (num_segments - 1) + [33]
    check_path_episode(runs, len(cam), num_segments)
