"""What writing annotated images costs: the draw and encode kernels, the host half per frame, and detect.py end to end with and without them.

1. Kernels: a batch of --batch resident 1024-px synthetic tiles with --dets-per-tile random boxes each (labels on, line thickness 3):
   the host's primitive building and binning (milliseconds per batch), aq_annotate_u8 and aq_image_jpeg_coefs timed between HIP events over
   --reps launches (microseconds per batch).
2. Host: aq_write_image_files on eight of those frames into a scratch directory (no fsync; 4 threads, as detect.py calls it), and
   aq_image_jpeg_bytes on one thread: microseconds per frame and per block, for the synthetic tiles and for random pixels (the coder's worst case).
3. detect.py --quiet --save-txt --save-conf on --tiles synthetic 1024-px JPEG tiles (split decode, bf16), with --nosave and without, at two
   confidence thresholds (two detection densities), two interleaved runs each: images/s as the run reports it.

    python tools/bench_save_img.py [--batch 64] [--dets-per-tile 340] [--tiles 512] [--conf 0.25 0.9]

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


def kernels_and_host(batch, per_tile, reps, size=1024):
    import torch
    from aquaculture_amd import annotate, engine, postprocess, tiles
    lib = engine.load_library()
    rng = np.random.default_rng(0)
    host = np.stack([tiles.synthetic_tile(i % 36, size) for i in range(batch)])
    imgs = torch.from_numpy(host).cuda()
    n = batch * per_tile
    wh = rng.integers(10, 200, (n, 2))
    x1, y1 = rng.integers(0, size - wh[:, 0] + 1), rng.integers(0, size - wh[:, 1] + 1)
    xyxy = np.stack([x1, y1, x1 + wh[:, 0], y1 + wh[:, 1]], 1)
    cls, conf = rng.integers(0, 5, n), rng.uniform(0.25, 1, n).astype(np.float32)
    owner = np.repeat(np.arange(batch), per_tile)
    sizes = [(size, size)] * batch
    names = ["circle_farms", "square_farms", "mussel_lines", "oyster_tables", "fish_cages"]
    atlas = annotate.LabelAtlas(imgs.device)
    atlas.lookup(postprocess.label_strings(names, cls, conf), annotate.font_size(size, size))       # rasterised once per sweep, not per batch
    t = time.perf_counter()
    labels = atlas.lookup(postprocess.label_strings(names, cls, conf), annotate.font_size(size, size))
    P, img = postprocess.annotation_prims(owner, cls, xyxy, sizes, 3, labels)
    t_prims = time.perf_counter() - t
    cs, cp = postprocess.bin_prims(P, img, sizes)
    t_bins = time.perf_counter() - t - t_prims
    prims = postprocess.prims_array(P, engine.PRIM_DTYPE)
    canvases, nbytes = engine.canvas_table(np.arange(batch) * size * size * 3, size * 3, sizes)
    out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(3):
            fn()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    # (annotate_images uploads its tables on every call, as detect.py does: the time is that of the call, not of the kernel alone)
    us_draw_call = timed(lambda: engine.annotate_images(imgs.view(-1), canvases, prims, cs, cp, atlas.device_atlas(), nbytes, out=out))
    table = engine.frame_table(canvases["dst"], canvases["dst_pitch"], sizes)
    nm = int(engine.frame_mcus(table).sum())
    arena = torch.empty(nm * 384, dtype=torch.int16, device="cuda")
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    st = torch.cuda.current_stream()
    us_encode = timed(lambda: lib.aq_image_jpeg_coefs(out.data_ptr(), out.numel(), table_dev.data_ptr(), table.ctypes.data, batch, nm, arena.data_ptr(),
                                                       st.cuda_stream))
    res = {"batch": batch, "dets_per_tile": per_tile, "prims": int(prims.shape[0]), "cell_entries": int(cp.shape[0]),
           "host_prims_ms_per_batch": round(t_prims * 1e3, 1), "host_bins_ms_per_batch": round(t_bins * 1e3, 1),
           "draw_call_us_per_batch": round(us_draw_call, 1), "encode_kernel_us_per_batch": round(us_encode, 1), "mcus": nm}
    k = min(batch, 8)
    for kind, src in (("synthetic", out), ("random", torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda"))):
        coef, tab = engine.encode_frames(src, table[:k])
        rel = [f"t{i}.jpg" for i in range(k)]
        with tempfile.TemporaryDirectory() as d:
            engine.write_image_files(d, rel, coef, tab, threads=4)
            t = time.perf_counter()
            engine.write_image_files(d, rel, coef, tab, threads=4)
            us_files = (time.perf_counter() - t) * 1e6 / k
            nb = sum(os.path.getsize(os.path.join(d, r)) for r in rel) / k
        t = time.perf_counter()
        per = (size // 16) ** 2
        for i in range(k):
            engine.image_jpeg_bytes(coef[i * per:(i + 1) * per], size, size)
        us_one = (time.perf_counter() - t) * 1e6 / k
        res[kind] = {"host_us_per_frame_files_4_threads": round(us_files, 1), "host_us_per_frame_bytes_1_thread": round(us_one, 1),
                     "host_us_per_block_1_thread": round(us_one / (per * 6), 3), "mean_file_bytes": int(nb)}
    return res


def detect_runs(n_tiles, confs, batch):
    import shutil
    from aquaculture_amd import checkpoint, tiles
    out = []
    with tempfile.TemporaryDirectory() as d:
        tiles.write_synthetic_jpegs(os.path.join(d, "jpegs"), range(n_tiles), size=1024)
        w = os.path.join(d, "synth.pt")
        checkpoint.write_synthetic_checkpoint(w, "yolov5m", 5)
        for conf in confs:
            for save in (False, True, False, True):                      # interleaved, twice each
                name = f"c{conf}_{int(save)}_{len(out)}"
                cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", w, "--source", os.path.join(d, "jpegs"),
                       "--save-txt", "--save-conf", "--quiet", "--half", "--jpeg-decode", "split", "--batch-size", str(batch), "--conf-thres", str(conf),
                       "--project", os.path.join(d, "runs"), "--name", name, *([] if save else ["--nosave"])]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
                ips = float(re.search(r"([0-9.]+) images/s on", r.stdout).group(1))
                steady = re.search(r"steady state: ([0-9.]+) images/s", r.stdout)
                dets = int(re.search(r"images, (\d+) detections", r.stdout).group(1))
                out.append({"conf": conf, "save_img": save, "images_s": ips, "steady_images_s": float(steady.group(1)) if steady else None,
                            "dets_per_tile": round(dets / n_tiles, 1)})
                shutil.rmtree(os.path.join(d, "runs", name))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dets-per-tile", type=int, default=340)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tiles", type=int, default=512)
    ap.add_argument("--conf", type=float, nargs="+", default=[0.25, 0.9])
    ap.add_argument("--skip-detect", action="store_true")
    args = ap.parse_args()
    from aquaculture_amd.build import build
    build()
    res = {"kernels_host": kernels_and_host(args.batch, args.dets_per_tile, args.reps)}
    if not args.skip_detect:
        res["detect"] = detect_runs(args.tiles, args.conf, args.batch)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
