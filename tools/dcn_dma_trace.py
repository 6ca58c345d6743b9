#!/usr/bin/env python3
"""Cycle-stamp timeline of one DCN forward launch inside the EDVR forward (debug build:
python -m dynavsr_amd.build --trace).  usage (GPU box): python tools/dcn_dma_trace.py [dcn_launch_index [H W]]
Stamps (thread 0 of each workgroup, chunks 0 and 1): 0 start; per chunk c: 1+30c top, 2+30c, 3+30c, 4+30c operands of
tap 0 ready, 5+30c+t tap t done; 62 loop done, 63 stores issued.  Stamps 2 and 3 by kernel:
  mdcn_fwd_split_kernel (two window buffers; the window DMAs of chunk c ride under taps 0-5 of chunk c - 1, the
  chunk's one barrier and the sampler of the next chunk's tap 0 are inside tap 8): chunk 0, whose window the prologue
  drains ahead of stamp 1: 2 = tap 0's A fragments requested, 3 = the first barrier passed, 4 = tap 0 sampled with
  nothing to hide it behind; chunk 1: 32 = 33 = top, 34 = the operands prepared under tap 8 copied to the even sets;
  mdcn_fwd_dma_kernel (DVSR_DCN_FWD=dma; one window buffer): 2+30c = first barrier passed and DMAs issued, 3+30c =
  second barrier passed (everything landed).
The columns keep their places, so that the budgets of the two forms can be laid side by side."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("DVSR_HIP_LIB", os.path.join(HERE, "dynavsr_amd", "libdynavsr_hip_trace.so"))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dynavsr_amd import _lib, engine, synth  # noqa: E402
from dynavsr_amd.models.archs.EDVR_arch import EDVR  # noqa: E402

idx = int(sys.argv[1]) if len(sys.argv) > 1 else 2
h = int(sys.argv[2]) if len(sys.argv) > 3 else 180
w = int(sys.argv[3]) if len(sys.argv) > 3 else 320
net = EDVR()
net.load_state_dict(synth.edvr_state_dict(0))
net = net.cuda()
x = synth.clip(1, 1, 5, h, w, smooth=False).cuda()
plan = engine.get_plan(net._cfg(), 1, h, w)
params = [p.detach().contiguous() for p in net.ordered_parameters()]
ws = torch.empty(plan.workspace_bytes(False), dtype=torch.uint8, device="cuda")
out = torch.empty(1, 3, 4 * h, 4 * w, device="cuda")
for _ in range(2):
    plan.forward(params, x, out, ws)
torch.cuda.synchronize()
NB = 1 << 14
buf = torch.zeros(NB * 64, dtype=torch.int64, device="cuda")
fn = _lib.lib().dvsr_debug_dcn_trace
fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
fn(buf.data_ptr(), idx)
plan.forward(params, x, out, ws)
torch.cuda.synchronize()
t = buf.cpu().numpy().reshape(NB, 64)
t = t[t[:, 0] != 0]
print("workgroups traced: %d; launch span %.0f cycles" % (len(t), float(t[:, 63].max() - t[:, 0].min())))
med = lambda v: float(np.median(v))
print("lifetime                      %8.0f cycles (median)" % med(t[:, 63] - t[:, 0]))
print("start -> first chunk top      %8.0f" % med(t[:, 1] - t[:, 0]))
for c in range(2):
    b = 30 * c
    # (split kernel, chunk 1: nothing | nothing | the operand copies; its barrier and tap 0's sampler are inside tap 8 of chunk 0)
    print("chunk %d: barrier 1 + DMA issue %6.0f | DMA landed (barrier 2) %6.0f | tap 0 operands %6.0f" % (
        c, med(t[:, b + 2] - t[:, b + 1]), med(t[:, b + 3] - t[:, b + 2]), med(t[:, b + 4] - t[:, b + 3])))
    taps = [med(t[:, b + 5 + k] - t[:, b + 4 + k]) for k in range(9)]
    print("   taps (16 MFMAs = 1024 cycles + the next tap's sampler):", " ".join("%5.0f" % v for v in taps))
print("chunk 0 top -> chunk 1 top    %8.0f" % med(t[:, 31] - t[:, 1]))
print("epilogue %6.0f" % med(t[:, 63] - t[:, 62]))
