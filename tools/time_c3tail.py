#!/usr/bin/env python3
"""A/B timing at batch 64, 640-px tiles (model.2 runs at 160 x 160): aq_bottleneck (C = 48) + aq_conv1x1_direct (96 -> 96) -- model.2.m.1 and
model.2.cv3 as two launches -- against aq_bottleneck_c3tail (one), interleaved.  python tools/time_c3tail.py [B]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from aquaculture_amd import engine as E

lib = E.load_library()
dev = torch.device("cuda", 0)
B, H, W = int(sys.argv[1]) if len(sys.argv) > 1 else 64, 160, 160
g = torch.Generator().manual_seed(0)
fp = C.POINTER(C.c_float)
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr())
nbuf = 3                                                 # rotating buffers: every launch reads HBM-cold data, as in the engine
xs = [torch.randn(B, H, W, 48, generator=g).to(torch.bfloat16).to(dev) for _ in range(nbuf)]
cats = [torch.randn(B, H, W, 96, generator=g).to(torch.bfloat16).to(dev) for _ in range(nbuf)]
outs = [torch.empty((B, H, W, 96), dtype=torch.bfloat16, device=dev) for _ in range(nbuf)]
w1 = np.ascontiguousarray((torch.randn(48, 1, 1, 48, generator=g) * 0.2).numpy())
w2 = np.ascontiguousarray((torch.randn(48, 3, 3, 48, generator=g) * 0.07).numpy())
w3 = np.ascontiguousarray((torch.randn(96, 1, 1, 96, generator=g) * 0.14).numpy())
n = C.c_size_t()
E._check(lib.aq_pack_bottleneck_weights(w1.ctypes.data_as(fp), w2.ctypes.data_as(fp), 48, None, C.byref(n), None))
wb = torch.empty(n.value, dtype=torch.uint8, device=dev)
E._check(lib.aq_pack_bottleneck_weights(w1.ctypes.data_as(fp), w2.ctypes.data_as(fp), 48, vp(wb), C.byref(n), st()))
E._check(lib.aq_pack_conv1x1_direct(w3.ctypes.data_as(fp), 96, 96, None, C.byref(n), None))
wc = torch.empty(n.value, dtype=torch.uint8, device=dev)
E._check(lib.aq_pack_conv1x1_direct(w3.ctypes.data_as(fp), 96, 96, vp(wc), C.byref(n), st()))
E._check(lib.aq_pack_bottleneck_c3tail_weights(w1.ctypes.data_as(fp), w2.ctypes.data_as(fp), w3.ctypes.data_as(fp), None, C.byref(n), None))
wt = torch.empty(n.value, dtype=torch.uint8, device=dev)
E._check(lib.aq_pack_bottleneck_c3tail_weights(w1.ctypes.data_as(fp), w2.ctypes.data_as(fp), w3.ctypes.data_as(fp), vp(wt), C.byref(n), st()))
bb = torch.randn(96, generator=g).to(dev) * 0.1
bc = torch.randn(96, generator=g).to(dev) * 0.1
bt = torch.cat([bb, bc])


def two(i):
    x, cat, out = xs[i % nbuf], cats[i % nbuf], outs[i % nbuf]
    E._check(lib.aq_bottleneck(vp(x), 48, 0, vp(cat), 96, 0, 48, vp(wb), vp(bb), B, H, W, 1, st()))
    E._check(lib.aq_conv1x1_direct(vp(cat), 96, 0, vp(out), 96, 0, 96, 96, vp(wc), vp(bc), B * H * W, 1, st()))


def one(i):
    x, cat, out = xs[i % nbuf], cats[i % nbuf], outs[i % nbuf]
    E._check(lib.aq_bottleneck_c3tail(vp(x), 48, 0, vp(cat), 96, 48, vp(out), 96, 0, vp(wt), vp(bt), B, H, W, 1, st()))


def timeit(fn, reps=20):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


# the fused output against the two launches' (same buffers: the two-launch form overwrites the concat's first half, which the fused form ignores)
one(0)
ref = outs[0].clone()
two(0)
torch.cuda.synchronize()
print(f"B={B}  fused == two launches: {torch.equal(ref, outs[0])}", flush=True)
for name, fn in (("bottleneck + cv3 1x1", two), ("c3tail (fused)", one)) * 3:
    print(f"B={B}  {name:22s} {timeit(fn):8.1f} us", flush=True)
