#!/usr/bin/env python3
"""What --blank-key costs.

  kernel   aq_blank_stats_u8 on a batch of 64 tiles of 1024 px in HBM: HIP events around 50 calls after warm-up, microseconds per call and
           bytes read per second; the yardstick beside it is aq_letterbox_u8 on the same batch (it reads the same source bytes and also writes).
  sweep    detect.py over a directory of synthetic 1024-px JPEG tiles with and without --blank-key, interleaved, `--runs` each: the steady-state
           images/s each run prints.

    python tools/bench_blank_key.py [--tiles 2048] [--runs 2] [--skip-sweep] [--out result.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_times(batch=64, size=1024, calls=50):
    import numpy as np
    import torch
    from aquaculture_amd.engine import blank_frame_table, blank_stats, letterbox_device, load_library
    lib = load_library()
    g = torch.Generator(device="cuda").manual_seed(1)
    tiles = torch.randint(0, 256, (batch, size, size, 3), generator=g, device="cuda", dtype=torch.uint8)
    tiles[:, :, size - 100:] = 255                          # a white margin: rows, columns and the box all have work
    table = blank_frame_table(np.arange(batch, dtype=np.int64) * size * size * 3, size * 3, [(size, size)] * batch)
    scratch = torch.empty(int(lib.aq_blank_stats_scratch_bytes(table.ctypes.data, batch)), dtype=torch.uint8, device="cuda")
    out = torch.empty((batch, 9), dtype=torch.int32, device="cuda")
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls            # microseconds per call

    us_stats = timed(lambda: blank_stats(tiles.view(-1), table, scratch=scratch, out=out, frames_dev=table_dev))
    us_letterbox = timed(lambda: letterbox_device(tiles, (640, 640), 32, True))
    nbytes = batch * size * size * 3
    return {"batch": batch, "tile": size, "calls": calls, "blank_stats_us": round(us_stats, 1), "letterbox_us": round(us_letterbox, 1),
            "bytes_read": nbytes, "blank_stats_TB_per_s": round(nbytes / us_stats / 1e6, 3),
            "letterbox_source_TB_per_s": round(nbytes / us_letterbox / 1e6, 3)}


def sweep_rates(n_tiles, runs, batch=64):
    from aquaculture_amd import checkpoint, tiles
    rates = {"plain": [], "blank_key": []}
    with tempfile.TemporaryDirectory() as d:
        tiles.write_synthetic_jpegs(os.path.join(d, "jpegs"), list(range(n_tiles)), size=1024)
        checkpoint.write_synthetic_checkpoint(os.path.join(d, "w.pt"), "yolov5m", 5)
        for r in range(runs):
            for kind, extra in (("plain", ()), ("blank_key", ("--blank-key",))):
                cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", os.path.join(d, "w.pt"), "--source",
                       os.path.join(d, "jpegs"), "--save-txt", "--save-conf", "--nosave", "--quiet", "--half", "--project", os.path.join(d, "runs"),
                       "--name", f"{kind}{r}", "--batch-size", str(batch), "--autotune", "off", *extra]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    raise RuntimeError(p.stdout[-2000:] + p.stderr[-2000:])
                m = re.search(r"steady state: ([0-9.]+) images/s", p.stdout)
                rates[kind].append(float(m.group(1)) if m else None)
    return {"tiles": n_tiles, "batch": batch, "steady_images_per_s": rates}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_blank_key needs a GPU: there is nothing to measure without one")
    res = {"kernel": kernel_times()}
    print(json.dumps(res["kernel"]), flush=True)
    if not a.skip_sweep:
        res["sweep"] = sweep_rates(a.tiles, a.runs)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
