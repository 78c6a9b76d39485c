"""GTM random access, host side (no GPU): tiler_gtm_seek moves the position and refuses frames outside the stream,
tiler_gtm_frames checks its whole list before it asks for a device, and tiler_debug_gtm_seek refuses negative sizes.
The pictures are tests/test_gpu_gtm_seek.py's."""
import numpy as np
import pytest

import gtm_player_cases as cases
from tiler_amd import TilerError, gtm, load


@pytest.fixture()
def small():
    with gtm.Stream(cases.case("small")["data"]) as st:
        yield st


def test_seek_moves_the_position(small):
    F = small.frames
    assert F == 9 and small.next_frame == 0
    for f in list(range(F + 1)) + [4, 4, 0]:
        small.seek(f)
        assert small.next_frame == f


@pytest.mark.parametrize("bad", [-1, 10])
def test_seek_outside_the_stream(small, bad):
    assert bad in (-1, small.frames + 1)
    small.seek(5)
    with pytest.raises(TilerError, match=rf"frame {bad} is outside \[0, 9\]"):
        small.seek(bad)
    assert small.next_frame == 5


def test_frames_of_an_empty_list(small):
    for layout, shape in (("tiles", (0, 35, 64)), ("raster", (0, 40, 56))):
        rgb, undrawn = small.frames([], layout)
        assert rgb.shape == shape and rgb.dtype == np.uint32
        assert undrawn.shape == (0,) and undrawn.dtype == np.int32
    assert small.frames_dev([], 0) == 0 and small.next_frame == 0


@pytest.mark.parametrize("indices, entry, value", [([9], 0, 9), ([0, -1], 1, -1)])
def test_frames_checks_the_list_before_the_device(small, indices, entry, value):
    """The range error, naming the entry and its value -- on a machine without a GPU too, where anything that reached
    for the device would report that instead."""
    for call in (lambda: small.frames(indices), lambda: small.frames(indices, chunk=1),
                 lambda: small.frames_dev(indices, 0)):
        with pytest.raises(TilerError) as e:
            call()
        assert f"frames[{entry}] = {value} is outside [0, 9)" in str(e.value)
    assert small.next_frame == 0


def test_debug_setter_rejects_negative_sizes():
    lib = load()
    assert lib.tiler_debug_gtm_seek(-1, 0) == -1 and lib.tiler_debug_gtm_seek(0, -1) == -1
    assert lib.tiler_debug_gtm_seek(0, 0) == 0
