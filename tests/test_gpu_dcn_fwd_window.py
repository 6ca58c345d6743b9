"""mdcn_fwd_split_kernel with two window buffers and offsets / masks read from global memory into registers.

The kernel walks the input in 8-channel chunks.  Chunk kc + 1's window is DMA-ed into the buffer chunk kc - 1 has left
while chunk kc's taps run, one raw barrier per chunk orders the two, and every tap's (dh, dw, mask) triple is loaded two
taps ahead, across the chunk boundary, from the planes of group kc / sub.  The cases below are the smallest at which that
structure can go wrong: one chunk (no next buffer), two (one swap), an odd count, sub = 2 (two chunks share a group's
planes), ragged tiles (lanes without a pixel must read 0), surplus workgroups that leave before any barrier, two cout
blocks, windows whose halo is in the image on one side only, and the sampling-gate case whose +-50 offsets send every
sample of two rows through the global fix-up.

Reference: the fp64 oracle each case of tests/test_gpu_dcn.py carries; bar: that file's TOL (relative L2).  Both
instantiations run: 'fast' reads masks, 'packfast' reads mask logits ('pack', the generic gather kernel on the same logits,
runs beside them).  Offsets are N(0, 2^2) against a 4-pixel halo, so a
wrong group index, buffer parity or stale window shows as an error of order 1.
"""
import pytest
import torch

from test_gpu_dcn import TOL, _id, check, gpu_forward, make_case

pytestmark = pytest.mark.gpu

# n, c, dg, cout, h, w (stride = pad = dil = 1), gate
CASES = [
    ((1, 8, 1, 64, 8, 32), False),       # one chunk
    ((1, 16, 2, 64, 8, 32), False),      # two chunks: one buffer swap
    ((1, 24, 3, 64, 9, 36), False),      # odd chunk count, ragged H, a 4-pixel-wide last tile column
    ((1, 32, 2, 64, 10, 40), False),     # sub = 2
    ((1, 128, 8, 64, 12, 36), False),    # sub = 2 at 16 chunks
    ((2, 64, 8, 64, 12, 36), False),     # EDVR's configuration, batch strides, partial tiles
    ((3, 64, 8, 64, 8, 32), False),      # three full tiles: five of the eight interleaved workgroup slots return early
    ((1, 64, 8, 128, 12, 36), False),    # two cout blocks
    ((1, 64, 8, 64, 17, 68), False),     # three tile rows and columns
    ((1, 64, 8, 64, 10, 36), True),      # exact gate boundaries, +-50 offsets
]


def _case(case, gate):
    return make_case(*case, 1, 1, 1, gate=gate)


@pytest.mark.parametrize("case,gate", CASES, ids=[_id(c) + ("-gate" if g else "") for c, g in CASES])
def test_window_forward(case, gate):
    cs = _case(case, gate)
    assert TOL == 2e-5
    check("window " + _id(case) + (" gate" if gate else ""), {k: gpu_forward(cs, k) for k in ("fast", "pack", "packfast")},
          {"fast": cs["out"], "pack": cs["out_pack"], "packfast": cs["out_pack"]})


def test_window_forward_repeatable():
    """A, B, A again: the three results of A are bit-equal, so nothing depends on what an earlier launch left in the LDS
    (both window buffers' out-of-image slots are zeroed by every workgroup, every other slot is written before it is read)."""
    a, b = _case(*CASES[2]), _case(*CASES[8])
    for kind in ("fast", "pack", "packfast"):
        first = gpu_forward(a, kind)
        second = gpu_forward(a, kind)
        gpu_forward(b, kind)
        third = gpu_forward(a, kind)
        assert torch.equal(first, second) and torch.equal(first, third), kind
