"""What --save-crop costs: the encode kernel, the host half per crop, and detect.py end to end with and without the flag.

1. Kernel: a batch of --batch resident 1024-px tiles with --crops-per-tile crops each (sides 40-260 px, anywhere), aq_crop_jpeg_coefs timed
   between HIP events over --reps launches: microseconds per batch and per 1,000 block positions (a position = 8 x 8 pixels, Y / Cb / Cr).
2. Host: aq_write_crop_files on those coefficients into a scratch directory (no fsync; 4 threads, as detect.py calls it), and
   aq_crop_jpeg_bytes on one thread: microseconds per crop.
3. detect.py --quiet --save-txt --save-conf on --tiles synthetic 1024-px JPEG tiles (split decode, bf16), without and with --save-crop, at two
   confidence thresholds (two detection densities): images/s as the run reports it, and crops per tile.

    python tools/bench_save_crop.py [--batch 64] [--crops-per-tile 4] [--tiles 512] [--conf 0.6 0.9]

Prints one JSON line.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_and_host(batch, per_tile, reps, size=1024):
    import torch
    from aquaculture_amd import engine
    lib = engine.load_library()
    rng = np.random.default_rng(0)
    imgs = torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, device="cuda")
    n = batch * per_tile
    wh = rng.integers(40, 261, (n, 2))
    x1 = rng.integers(0, size - wh[:, 0] + 1)
    y1 = rng.integers(0, size - wh[:, 1] + 1)
    rects = np.stack([x1, y1, x1 + wh[:, 0], y1 + wh[:, 1]], 1)
    table = engine.crop_table(np.repeat(np.arange(batch), per_tile) * size * size * 3, size * 3, rects)
    nblk = int(engine.crop_blocks(table).sum())
    coef, _ = engine.encode_crops(imgs.view(-1), table, arena_blocks=max(nblk, 1))
    arena = torch.empty(nblk * 192, dtype=torch.int16, device="cuda")
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    st = torch.cuda.current_stream()
    launch = lambda: lib.aq_crop_jpeg_coefs(imgs.data_ptr(), imgs.numel(), table_dev.data_ptr(), n, nblk, arena.data_ptr(), st.cuda_stream)
    for _ in range(5):
        assert launch() == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    rel = [f"crops/c{i % 5}/t{i // per_tile}_{i % per_tile}.jpg" for i in range(n)]
    with tempfile.TemporaryDirectory() as d:
        engine.write_crop_files(d, rel, coef, table, threads=4)          # directories exist from here on, as in a running sweep
        t = time.perf_counter()
        engine.write_crop_files(d, rel, coef, table, threads=4)
        us_files = (time.perf_counter() - t) * 1e6 / n
        nbytes = sum(os.path.getsize(os.path.join(d, r)) for r in rel)
    t = time.perf_counter()
    for i in range(n):
        b, w, h = int(table["block"][i]), int(rects[i, 2] - rects[i, 0]), int(rects[i, 3] - rects[i, 1])
        engine.crop_jpeg_bytes(coef[b:b + ((w + 7) // 8) * ((h + 7) // 8)], w, h)
    us_bytes = (time.perf_counter() - t) * 1e6 / n
    return {"batch": batch, "crops": n, "blocks": nblk, "kernel_us_per_batch": round(us, 1), "kernel_us_per_1k_blocks": round(us * 1e3 / nblk, 2),
            "host_us_per_crop_files_4_threads": round(us_files, 1), "host_us_per_crop_bytes_1_thread": round(us_bytes, 1),
            "mean_file_bytes": int(nbytes / n)}


def detect_runs(n_tiles, confs, batch):
    from aquaculture_amd import checkpoint, tiles
    out = []
    with tempfile.TemporaryDirectory() as d:
        tiles.write_synthetic_jpegs(os.path.join(d, "jpegs"), range(n_tiles), size=1024)
        w = os.path.join(d, "synth.pt")
        checkpoint.write_synthetic_checkpoint(w, "yolov5m", 5)
        for conf in confs:
            for crop in (False, True, False, True):                      # interleaved, twice each
                name = f"c{conf}_{int(crop)}_{len(out)}"
                cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", w, "--source", os.path.join(d, "jpegs"), "--nosave",
                       "--save-txt", "--save-conf", "--quiet", "--half", "--jpeg-decode", "split", "--batch-size", str(batch), "--conf-thres", str(conf),
                       "--project", os.path.join(d, "runs"), "--name", name, *(["--save-crop"] if crop else [])]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
                ips = float(re.search(r"([0-9.]+) images/s on", r.stdout).group(1))
                steady = re.search(r"steady state: ([0-9.]+) images/s", r.stdout)
                dets = int(re.search(r"images, (\d+) detections", r.stdout).group(1))
                ncrop = sum(len(f) for _, _, f in os.walk(os.path.join(d, "runs", name, "crops"))) if crop else 0
                out.append({"conf": conf, "save_crop": crop, "images_s": ips, "steady_images_s": float(steady.group(1)) if steady else None,
                            "dets_per_tile": round(dets / n_tiles, 1), "crops_per_tile": round(ncrop / n_tiles, 1)})
                import shutil
                shutil.rmtree(os.path.join(d, "runs", name))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--crops-per-tile", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--tiles", type=int, default=512)
    ap.add_argument("--conf", type=float, nargs="+", default=[0.6, 0.9])
    ap.add_argument("--skip-detect", action="store_true")
    args = ap.parse_args()
    from aquaculture_amd.build import build
    build()
    res = {"kernel_host": kernel_and_host(args.batch, args.crops_per_tile, args.reps)}
    if not args.skip_detect:
        res["detect"] = detect_runs(args.tiles, args.conf, args.batch)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
