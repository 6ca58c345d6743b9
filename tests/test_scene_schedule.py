"""CPU: windows that stay inside a scene (adapt.video_windows / stream_schedule(cuts=...)), the frame cache's capacity with
more than one scene, the validation of `cuts`, and the scene-change scores (frames.scene_scores / cut selection).

The windows are held to tests/golden/index_generation.json, the lists the reference's own index_generation returned: a
scene is what the reference's datasets read as one folder.  The capacity is held by simulation, and shown to be the
smallest by the same simulation with one slot fewer."""
import json
import os
import random

import numpy as np
import pytest

import cut_ref
from dynavsr_amd import frames as fio
from dynavsr_amd.adapt import scene_bounds, stream_schedule, stream_slots, video_windows
from dynavsr_amd.data.util import index_generation

MODES = ('replicate', 'reflection', 'new_info', 'circle')
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_generation.json")))


def scene_windows_by_the_rule(length, nframes, mode):
    """The windows of a scene of `length` frames that starts at 0, as the issue states them: the reference's lists where they
    exist, 'replicate' for a scene in which some window under `mode` would leave it."""
    if length >= nframes:
        return [GOLDEN["%d,%d,%d,%s" % (nframes, length, c, mode)] for c in range(length)]
    own = [index_generation(c, length, nframes, mode) for c in range(length)]
    if any(min(w) < 0 or max(w) >= length for w in own):
        return [index_generation(c, length, nframes, 'replicate') for c in range(length)]
    return own


@pytest.mark.parametrize("nframes", [3, 5, 7])
@pytest.mark.parametrize("mode", MODES)
def test_windows_of_a_scene_are_the_reference_lists(nframes, mode):
    short_seen = 0
    for first in (1, 2, nframes - 1, nframes, 9):
        for length in range(1, 13):
            for tail in (0, 3):
                cuts = [first] + ([first + length] if tail else [])
                T = first + length + tail
                wins, scenes = video_windows(T, nframes, mode, cuts)
                assert scenes == len(cuts) + 1 and len(wins) == T
                want = scene_windows_by_the_rule(length, nframes, mode)
                assert wins[first:first + length] == [[first + i for i in w] for w in want], (first, length, tail)
                short_seen += length < nframes
                for (a, b) in scene_bounds(T, cuts):
                    for c in range(a, b):
                        assert len(wins[c]) == nframes and wins[c][nframes // 2] == c
                        assert a <= min(wins[c]) and max(wins[c]) < b, (cuts, c, wins[c])
    assert short_seen


def test_short_scene_takes_replicate_only_where_the_mode_leaves_it():
    # reflection stays inside a scene of 3 frames at nframes = 5 (the case stream_schedule accepts today): it is kept
    wins, _ = video_windows(7, 5, 'reflection', [4])
    assert wins[4:] == [[4 + i for i in index_generation(c, 3, 5, 'reflection')] for c in range(3)]
    assert wins[4] == [6, 5, 4, 5, 6]
    # new_info does not: the whole scene takes replicate
    wins, _ = video_windows(7, 5, 'new_info', [4])
    assert wins[4:] == [[4, 4, 4, 5, 6], [4, 4, 5, 6, 6], [4, 5, 6, 6, 6]]
    # a 1-frame scene at the very start, a 2-frame flash in the middle
    wins, scenes = video_windows(12, 5, 'new_info', [1, 6, 8])
    assert scenes == 4 and wins[0] == [0] * 5 and wins[6] == [6, 6, 6, 7, 7] and wins[7] == [6, 6, 7, 7, 7]
    assert wins[1:6] == [[1 + i for i in GOLDEN["5,5,%d,new_info" % c]] for c in range(5)]


def simulate(windows, slots, in_flight):
    """The frame cache run on the CPU: frames extracted in increasing order when a window first needs them, frame f into
    slot f % slots.  Returns None, or what went wrong: an overwritten slot that the current window or one of the
    in_flight - 1 before it names, or a window whose slots do not hold its frames."""
    held, recent, done = {}, [], 0
    for c, win in enumerate(windows):
        live = set(win).union(*recent[len(recent) - (in_flight - 1):]) if in_flight > 1 else set(win)
        for f in range(done, max(done, max(win) + 1)):
            if held.get(f % slots) in live:
                return "centre %d: frame %d overwrites live frame %d" % (c, f, held[f % slots])
            held[f % slots] = f
        done = max(done, max(win) + 1)
        if [held.get(f % slots) for f in win] != win:
            return "centre %d: the slots hold %s, the window is %s" % (c, [held.get(f % slots) for f in win], win)
        recent.append(win)
    return None


def cut_sets(T, rng):
    sets = [[k] for k in range(1, T)] + [list(range(1, T))]
    for _ in range(4):
        sets.append(sorted(rng.sample(range(1, T), rng.randint(1, min(T - 1, 6)))))
    return sets


@pytest.mark.parametrize("nframes", [3, 5, 7])
@pytest.mark.parametrize("in_flight", [1, 2, 3, 4])
def test_capacity_with_cuts(nframes, in_flight):
    rng = random.Random(1000 * nframes + in_flight)
    want_slots = nframes if in_flight == 1 else 2 * nframes + in_flight - 2
    assert stream_slots(nframes, in_flight, 2) == want_slots and stream_slots(nframes, in_flight, 9) == want_slots
    assert stream_slots(nframes, in_flight, 1) == nframes + in_flight - 1
    fewer_fails = 0
    for mode in MODES:
        for T in range(2, 30):
            for cuts in cut_sets(T, rng):
                windows, scenes = video_windows(T, nframes, mode, cuts)
                assert scenes == len(cuts) + 1 > 1
                # the schedule itself, step by step
                held, recent, next_frame = {}, [], 0
                steps = list(stream_schedule(T, nframes, mode, in_flight, cuts))
                assert [s[0] for s in steps] == list(range(T))
                for (centre, new, pairs, wslots), win in zip(steps, windows):
                    live = set(win).union(*recent[len(recent) - (in_flight - 1):]) if in_flight > 1 else set(win)
                    assert [f for f, _ in pairs] == new
                    for f, slot in pairs:
                        assert f == next_frame, "frames are extracted in increasing order, each once"
                        next_frame += 1
                        assert slot == f % want_slots and 0 <= slot < want_slots
                        assert held.get(slot) not in live, (nframes, in_flight, T, mode, cuts, centre, f, held.get(slot))
                        held[slot] = f
                    assert len(wslots) == nframes
                    assert [held[s] for s in wslots] == win, (nframes, in_flight, T, mode, cuts, centre)
                    recent.append(win)
                assert next_frame == T, "every frame is extracted exactly once"
                # the same rule in the stand-alone simulation, at the capacity and with one slot fewer
                assert simulate(windows, want_slots, in_flight) is None
                fewer_fails += simulate(windows, want_slots - 1, in_flight) is not None
    if in_flight >= 2:
        assert fewer_fails >= 1, "capacity - 1 never failed: the stated capacity is not the smallest"


PARENT = {      # what stream_schedule yielded before it knew of cuts
    (6, 5, 'new_info', 2): [(0, [0, 1, 2, 3, 4], [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)], [4, 3, 0, 1, 2]), (1, [], [], [4, 0, 1, 2, 3]),
                            (2, [], [], [0, 1, 2, 3, 4]), (3, [5], [(5, 5)], [1, 2, 3, 4, 5]), (4, [], [], [2, 3, 4, 5, 1]),
                            (5, [], [], [3, 4, 5, 2, 1])],
    (4, 3, 'circle', 3): [(0, [0, 1, 2], [(0, 0), (1, 1), (2, 2)], [2, 0, 1]), (1, [], [], [0, 1, 2]), (2, [3], [(3, 3)], [1, 2, 3]),
                          (3, [], [], [2, 3, 1])],
    (5, 3, 'replicate', 1): [(0, [0, 1], [(0, 0), (1, 1)], [0, 0, 1]), (1, [2], [(2, 2)], [0, 1, 2]), (2, [3], [(3, 0)], [1, 2, 0]),
                             (3, [4], [(4, 1)], [2, 0, 1]), (4, [], [], [0, 1, 1])],
    (7, 5, 'reflection', 2): [(0, [0, 1, 2], [(0, 0), (1, 1), (2, 2)], [2, 1, 0, 1, 2]), (1, [3], [(3, 3)], [1, 0, 1, 2, 3]),
                              (2, [4], [(4, 4)], [0, 1, 2, 3, 4]), (3, [5], [(5, 5)], [1, 2, 3, 4, 5]), (4, [6], [(6, 0)], [2, 3, 4, 5, 0]),
                              (5, [], [], [3, 4, 5, 0, 5]), (6, [], [], [4, 5, 0, 5, 4])],
}


def test_no_cuts_is_the_schedule_of_before():
    for args, want in PARENT.items():
        assert list(stream_schedule(*args)) == want
        assert list(stream_schedule(*args, cuts=None)) == want
        assert list(stream_schedule(*args, cuts=[])) == want
    # cuts=None keeps raising for a video that is too short; scene mode never raises for one
    for mode in ('new_info', 'circle'):
        for T in range(1, 5):
            with pytest.raises(ValueError):
                list(stream_schedule(T, 5, mode, 2))
            steps = list(stream_schedule(T, 5, mode, 2, cuts=[]))
            assert steps == list(stream_schedule(T, 5, 'replicate', 2))
    # cuts=[] equals today's call wherever today's call does not raise
    for nframes in (3, 5, 7):
        for mode in MODES:
            for T in range(1, 16):
                for k in (1, 2, 3):
                    try:
                        want = list(stream_schedule(T, nframes, mode, k))
                    except ValueError:
                        continue
                    assert list(stream_schedule(T, nframes, mode, k, cuts=[])) == want


@pytest.mark.parametrize("cuts", [[5, 3], [3, 3], [0], [0, 4], [10], [4, 10], [2.0], [3.5], ['4'], [True], [None], 4, 'auto', '45',
                                  [-1], [[3]]])
def test_bad_cuts_raise(cuts):
    with pytest.raises(ValueError):
        list(stream_schedule(10, 5, 'new_info', 2, cuts=cuts))
    with pytest.raises(ValueError):
        video_windows(10, 5, 'new_info', cuts)


def test_good_cuts_of_other_sequence_types():
    want = list(stream_schedule(10, 5, 'new_info', 2, cuts=[3, 7]))
    assert list(stream_schedule(10, 5, 'new_info', 2, cuts=(3, 7))) == want
    assert list(stream_schedule(10, 5, 'new_info', 2, cuts=np.array([3, 7]))) == want
    assert list(stream_schedule(10, 5, 'new_info', 2, cuts=iter([3, 7]))) == want
    assert scene_bounds(10, [3, 7]) == [(0, 3), (3, 7), (7, 10)] and scene_bounds(10, []) == [(0, 10)]
    with pytest.raises(ValueError):
        list(stream_schedule(10, 5, 'zeros', 2, cuts=[3]))


def test_super_resolve_frames_checks_cuts_before_any_gpu_call():
    import torch
    from dynavsr_amd import adapt

    class Net(torch.nn.Module):          # (not EDVR: the per-clip branch; a forward would fail, none may be reached)
        nframes = 3

        def forward(self, x):
            raise AssertionError("reached the network")

    video = torch.zeros(6, 3, 8, 8)
    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    for bad in ([4, 2], [0], [6], [1.5], 'scenes'):
        with pytest.raises(ValueError):
            next(adapt.super_resolve_frames(opt, Net(), video, cuts=bad))


def test_scene_scores_by_hand():
    h, w = 10, 20
    full = 255 * h * w
    # a single spike: one cut, at the spike, and the frame after it scores low again
    sad = [0, full // 100, full // 100, full // 2, full // 100, 0]
    s = fio.scene_scores(sad, h, w)
    assert s.dtype.is_floating_point and s.element_size() == 8 and tuple(s.shape) == (7,)
    mafd = [0.0] + [100.0 * v / full for v in sad]
    want = [min(mafd[t], abs(mafd[t] - mafd[t - 1])) if t else 0.0 for t in range(7)]
    assert np.allclose(s.numpy(), want, rtol=0, atol=1e-12)
    assert np.allclose(s.numpy(), cut_ref.scene_scores(sad, h, w), rtol=0, atol=1e-12)
    assert [t for t in range(1, 7) if s[t] >= 10.0] == [4] == cut_ref.detect_cuts(sad, h, w, 10.0)
    assert abs(float(s[4]) - (50.0 - 1.0)) < 0.05 and float(s[5]) < 1.01
    # sustained fast motion: the difference is high but does not change -- no cut after the first frame pair
    sad = [full // 4] * 8
    s = fio.scene_scores(sad, h, w)
    assert [t for t in range(1, 9) if s[t] >= 10.0] == [1]
    assert float(s[1]) == pytest.approx(25.0, abs=0.05) and all(float(v) == 0.0 for v in s[2:])
    # the threshold is inclusive, and a full-scale flip scores 100
    s = fio.scene_scores([0, full, 0], h, w)
    assert float(s[2]) == 100.0 and float(s[3]) == 0.0 and float(s[0]) == 0.0
    assert cut_ref.detect_cuts([0, full, 0], h, w, 100.0) == [2]
    # no pairs: one frame, one score
    assert fio.scene_scores([], h, w).tolist() == [0.0]
    with pytest.raises(ValueError):
        fio.scene_scores([1], 0, 4)
