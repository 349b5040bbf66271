#!/usr/bin/env python3
"""The device half of the JPEG decode alone (aq_jpeg_idct_rgb / aq_jpeg_idct_rgb_checked): microseconds per call for a batch of tiles,
events around `calls` launches after a warm-up, `repeats` times -- the figures of DESIGN.md section 19.  A/B against another build of the
library: --lib PATH (or AQ_ENGINE_LIB), one process per library; --entry unchecked times aq_jpeg_idct_rgb, which every build has.

    python tools/time_jpeg_idct.py --entry checked
    python tools/time_jpeg_idct.py --entry unchecked --lib /path/to/another/libaqengine.so
"""
import argparse
import ctypes as C
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--entry", choices=("checked", "unchecked"), default="checked")
    ap.add_argument("--lib", default=os.environ.get("AQ_ENGINE_LIB"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from aquaculture_amd import build, jpeg, tiles
    build.build()
    lib = C.CDLL(a.lib or build.LIB)
    H = W = a.size
    n = jpeg.coef_count(H, W)
    coef = np.zeros((a.batch, n), np.int16)
    qt = np.zeros((a.batch, 3, 64), np.uint16)
    for i in range(min(a.batch, 8)):                        # eight distinct tiles, repeated: the kernels' time does not depend on the values
        bio = io.BytesIO()
        Image.fromarray(tiles.synthetic_tile(i, a.size)).save(bio, format="JPEG", quality=75)
        rc, _ = jpeg.decode_coeffs(bio.getvalue(), coef[i], qt[i])
        assert rc == 0
    for i in range(8, a.batch):
        coef[i], qt[i] = coef[i % 8], qt[i % 8]
    coef_d, qt_d = torch.from_numpy(coef).cuda(), torch.from_numpy(qt.view(np.int16)).cuda()
    off_d = (torch.arange(a.batch, dtype=torch.int64) * n).cuda()
    lib.aq_jpeg_scratch_bytes.restype = C.c_size_t
    lib.aq_jpeg_scratch_bytes.argtypes = [C.c_int] * 3
    scratch = torch.empty(lib.aq_jpeg_scratch_bytes(a.batch, H, W), dtype=torch.uint8, device="cuda")
    out = torch.empty((a.batch, H, W, 3), dtype=torch.uint8, device="cuda")
    flags = torch.empty(a.batch, dtype=torch.int32, device="cuda")
    vp, i32 = C.c_void_p, C.c_int
    stream = torch.cuda.current_stream().cuda_stream
    if a.entry == "checked":
        f = lib.aq_jpeg_idct_rgb_checked
        f.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
        call = lambda: f(coef_d.data_ptr(), off_d.data_ptr(), qt_d.data_ptr(), a.batch, H, W, scratch.data_ptr(), out.data_ptr(), flags.data_ptr(), stream)
    else:
        f = lib.aq_jpeg_idct_rgb
        f.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
        call = lambda: f(coef_d.data_ptr(), off_d.data_ptr(), qt_d.data_ptr(), a.batch, H, W, scratch.data_ptr(), out.data_ptr(), stream)

    def timed():
        for _ in range(5):
            assert call() == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls            # microseconds per call

    us = [round(timed(), 1) for _ in range(a.repeats)]
    if a.entry == "checked":
        assert not flags.any()
    print(json.dumps({"lib": a.lib or build.LIB, "entry": a.entry, "batch": a.batch, "tile": a.size, "calls": a.calls, "us_per_call": us,
                      "median_us": sorted(us)[len(us) // 2], "min_us": min(us), "max_us": max(us)}))


if __name__ == "__main__":
    main()
