# coding: utf-8
"""The north-star shape's operands (Conv1dGLU fwd, B=64 x 256 x 1024, k=3) and the event timer that bf16_stage1.py
and wgrad_ab.py import.  The A/B this file was written for -- the tap-GEMM that splits while staging
against the persistent planes kernel on fp32 inputs split by a pass of their own (the opt-in route of DESIGN.md 3.3) --
went with that route (DESIGN.md 3.3 keeps its result; git history keeps the script)."""
import math, sys, os
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepvoice3_pytorch_amd import ops, _lib

dev = torch.device("cuda:0")
B, C, T, k = 64, 256, 1024, 3
torch.manual_seed(0)
x = torch.randn(B, C, T, device=dev)
v = torch.randn(2 * C, C, k, device=dev) * math.sqrt(4.0 * 0.95 / (k * C))
g = v.reshape(2 * C, -1).norm(dim=1).view(-1, 1, 1).clone()
bias = torch.zeros(2 * C, device=dev)
lib = _lib.lib()


def timeit(fn, iters=50, settle=30):
    for _ in range(settle):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters
