"""CPU: the window indexing and the frame-cache schedule of the streaming video forward (adapt.super_resolve_frames).

index_generation is held to tests/golden/index_generation.json, the lists the reference's own function returned
(tools/gen_index_generation_golden.py recorded them); stream_schedule to its stated properties by simulation."""
import json
import os

import pytest

from dynavsr_amd.adapt import stream_schedule
from dynavsr_amd.data.util import index_generation

MODES = ('replicate', 'reflection', 'new_info', 'circle')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_generation.json")


def test_index_generation_matches_reference_lists():
    gold = json.load(open(GOLDEN))
    seen = 0
    for n in (3, 5, 7):
        for max_n in range(n, 13):
            for crt in range(max_n):
                for mode in MODES:
                    assert index_generation(crt, max_n, n, mode) == gold["%d,%d,%d,%s" % (n, max_n, crt, mode)], (n, max_n, crt, mode)
                    seen += 1
    assert seen == len(gold) == 800


def test_index_generation_docstring_examples_and_bad_mode():
    assert index_generation(0, 10, 5, 'replicate') == [0, 0, 0, 1, 2]
    assert index_generation(0, 10, 5, 'reflection') == [2, 1, 0, 1, 2]
    assert index_generation(0, 10, 5, 'new_info') == [4, 3, 0, 1, 2]
    assert index_generation(0, 10, 5, 'circle') == [3, 4, 0, 1, 2]
    assert index_generation(4, 10, 5) == [2, 3, 4, 5, 6]
    with pytest.raises(ValueError):
        index_generation(0, 10, 5, 'zeros')
    with pytest.raises(ValueError):
        index_generation(4, 10, 5, 'zeros')


@pytest.mark.parametrize("nframes", [3, 5, 7])
@pytest.mark.parametrize("in_flight", [1, 2, 3, 4])
def test_stream_schedule_properties(nframes, in_flight):
    slots = nframes + in_flight - 1
    for mode in MODES:
        for T in range(nframes, 40):
            held = {}                  # slot -> frame it holds
            recent = []                # windows of the steps before this one
            next_frame = 0
            steps = list(stream_schedule(T, nframes, mode, in_flight))
            assert [s[0] for s in steps] == list(range(T))
            for centre, new, pairs, wslots in steps:
                win = index_generation(centre, T, nframes, mode)
                # the windows that may still be running when this step's extractions are enqueued, and this one
                live = set(win).union(*recent[len(recent) - (in_flight - 1):]) if in_flight > 1 else set(win)
                assert [f for f, _ in pairs] == new
                for f, slot in pairs:
                    assert f == next_frame, "frames are extracted in increasing order, each once"
                    next_frame += 1
                    assert slot == f % slots and 0 <= slot < slots
                    assert held.get(slot) not in live, (nframes, in_flight, T, mode, centre, f, held.get(slot))
                    held[slot] = f
                assert len(wslots) == nframes
                assert [held[s] for s in wslots] == win, (nframes, in_flight, T, mode, centre)
                recent.append(win)
            assert next_frame == T, "every frame is extracted exactly once"


@pytest.mark.parametrize("mode", ['new_info', 'circle'])
def test_stream_schedule_short_video_raises(mode):
    for nframes in (3, 5, 7):
        for T in range(1, nframes):
            with pytest.raises(ValueError):
                list(stream_schedule(T, nframes, mode, 2))


def test_stream_schedule_short_video_accepted_where_indices_stay_inside():
    # replicate never leaves [0, T); reflection stays inside once T > nframes // 2
    for T in range(1, 5):
        steps = list(stream_schedule(T, 5, 'replicate', 2))
        assert len(steps) == T and sum(len(s[1]) for s in steps) == T
    assert len(list(stream_schedule(3, 5, 'reflection', 1))) == 3
    with pytest.raises(ValueError):
        list(stream_schedule(2, 5, 'reflection', 1))
    with pytest.raises(ValueError):
        list(stream_schedule(8, 5, 'zeros', 2))
