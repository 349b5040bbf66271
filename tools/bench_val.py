#!/usr/bin/env python3
"""What the device steps of yolov5/val.py cost on one MI355X.  Each figure: the median of `--repeats` (default
5) timed calls after two warm-ups, with minimum and maximum, by HIP events around the call on the current stream.

  expand    aq_val_expand_rows_f32 at 25,200 rows x 5 classes, batch 32 (the default val.py batch at 640 px), on a synthetic pred in which
            `--share` (default 0.02) of the rows have obj above the threshold, every class of such a row passing
  match     aq_val_match at 32 images x 300 detections x 20 labels, the detections scattered around the labels
  confusion aq_val_confusion (--confusion-matrix) on the match step's inputs: 32 images x 300 detections x 20 labels, 5 classes, the default
            thresholds 0.25 / 0.45; beside the match row, which is its comparison (same inputs, the same shape of kernel)
  scores    aq_val_scores_f64 (val.score_gpu: torch's two stable sorts, then the launcher) at 10^7 detections over 5 classes, against
            val.score_cpu -- the numpy restatement -- on the same host, once; the two results have to be the same bytes

With `--map DATA.yaml --weights W.pt`: val.py on that split under fp32, f16x3, bf16, fp8 and fp8w, mAP beside the sweep's images/s.

With `--plots` only the --plots leg runs, at 640 px and 16 images, 8 labels and 40 detections per image:
  mosaic, annotate, coefs   the aq_val_mosaic_u8 launch, the two aq_annotate_u8 launches and the aq_image_jpeg_coefs_q(75) launch over both frames
  plot_batch                the whole val_plots.plot_batch on the host clock (primitives, uploads, launches, read-back, Huffman coding, two files)
  pillow                    the same two files made on the host: paste, dataloader.resize_linear_u8, ImageDraw, Image.save
and, with `--map DATA.yaml --weights W.pt`, the fp32 sweep's images/s with and without --plots 3 on that split.

    python tools/bench_val.py [--repeats 5] [--share 0.02] [--detections 10000000] [--no-cpu] [--map DATA.yaml --weights W.pt] [--out result.json]
    python tools/bench_val.py --plots [--repeats 5] [--map DATA.yaml --weights W.pt] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "values": list(v)}


def timed(fn, repeats):
    import torch
    for _ in range(2):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return spread(out)


def pillow_plot(images, geo, paths, targets, names, fname):
    """plot_images on the host from the uint8 batch: paste, resize, upstream's Annotator calls, Image.save (the comparison of the --plots leg)."""
    import numpy as np
    from pathlib import Path
    from PIL import Image, ImageDraw
    from aquaculture_amd import annotate, dataloader, postprocess, val_plots
    H, W, h, w = geo["H"], geo["W"], geo["h"], geo["w"]
    mosaic = np.full((*geo["src_size"], 3), 255, np.uint8)
    for i in range(geo["n"]):
        x, y = geo["src_origins"][i]
        mosaic[y:y + H, x:x + W] = images[i]
    if geo["resized"]:
        mosaic = dataloader.resize_linear_u8(mosaic, geo["size"][1], geo["size"][0])
    lw, fs = val_plots.annotator_sizes(geo)
    im = Image.fromarray(mosaic)
    draw, font = ImageDraw.Draw(im), annotate.load_font(fs)
    for i in range(geo["n"]):
        x, y = (int(v) for v in geo["origins"][i])
        draw.rectangle([x, y, x + w, y + h], None, (255, 255, 255), 2)
        draw.text([x + 5, y + 5], Path(paths[i]).name[:40], fill=(220, 220, 220), font=font)
        t = targets[i]
        for j, box in enumerate(val_plots.cell_boxes(t, geo, i).tolist()):
            if t.shape[1] == 6 and not t[j, 5] > 0.25:
                continue
            colour = tuple(int(v) for v in postprocess.PALETTE[int(t[j, 0]) % 20])
            label = names[int(t[j, 0])] if t.shape[1] == 5 else f"{names[int(t[j, 0])]} {t[j, 5]:.1f}"
            draw.rectangle(box, width=lw, outline=colour)
            tw, th = font.getbbox(label)[2:]
            outside = box[1] - th >= 0
            draw.rectangle((box[0], box[1] - th if outside else box[1], box[0] + tw + 1, box[1] + 1 if outside else box[1] + th + 1), fill=colour)
            draw.text((box[0], box[1] - th if outside else box[1]), label, fill=(255, 255, 255), font=font)
    im.save(fname)


def plots_leg(opt, res):
    import numpy as np
    import torch
    from aquaculture_amd import val, val_plots
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    B, H, W, L, D = 16, 640, 640, 8, 40
    names = {i: f"class{i}" for i in range(5)}
    yy, xx = np.mgrid[0:H, 0:W]
    images = np.stack([np.stack([(xx + 7 * i) % 256, (yy * 2 + i) % 256, (xx + yy) // 5 % 256], 2) for i in range(B)]).astype(np.uint8)
    images ^= rng.integers(0, 32, images.shape, dtype=np.uint8)
    paths = [f"images/tile_{i:04d}.jpg" for i in range(B)]
    labels = [np.concatenate([rng.integers(0, 5, (L, 1)), rng.random((L, 2)) * 0.8 + 0.1, rng.random((L, 2)) * 0.2 + 0.03], 1).astype(np.float32)
              for _ in range(B)]
    dets = np.zeros((B, D, 6), np.float32)
    c, sz = rng.random((B, D, 2)) * 600 + 20, rng.random((B, D, 2)) * 80 + 10
    dets[..., :2], dets[..., 2:4], dets[..., 4], dets[..., 5] = c - sz / 2, c + sz / 2, np.sort(rng.random((B, D)), 1)[:, ::-1], rng.integers(0, 5, (B, D))
    ltg, ptg = val_plots.batch_targets(dets, np.full(B, D), labels, (1024, 1024), (H, W))
    tiles = torch.from_numpy(images).to(dev)
    files = ("val_batch0_labels.jpg", "val_batch0_pred.jpg")
    with tempfile.TemporaryDirectory() as tmp:
        stages = {"mosaic_ms": [], "annotate_ms": [], "coefs_ms": []}
        wall = []
        for k in range(2 + opt.repeats):
            t = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            geo = val_plots.plot_batch(tiles, paths, ltg, ptg, names, tmp, files, times=t)
            if k >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
                for key in stages:
                    stages[key].append(t[key])
        plain = []
        for k in range(2 + opt.repeats):                                        # without the event synchronisations of the stage timing
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val_plots.plot_batch(tiles, paths, ltg, ptg, names, tmp, files)
            if k >= 2:
                plain.append((time.perf_counter() - t0) * 1e3)
        host = []
        for k in range(1 + opt.repeats):
            t0 = time.perf_counter()
            for name, tg in zip(files, (ltg, ptg)):
                pillow_plot(images, geo, paths, tg, names, os.path.join(tmp, "pillow_" + name))
            if k >= 1:
                host.append((time.perf_counter() - t0) * 1e3)
        same = [open(os.path.join(tmp, f), "rb").read() == open(os.path.join(tmp, "pillow_" + f), "rb").read() for f in files]
        sizes = [os.path.getsize(os.path.join(tmp, f)) for f in files]
    res["plots"] = {"images": B, "H": H, "W": W, "labels_per_image": L, "detections_per_image": D, "mosaic": list(geo["size"]), "file_bytes": sizes,
                    "same_bytes_as_pillow": same, "coefs_ms_includes": "the launch, the read-back of the coefficients and its synchronisation"}
    res["plots_mosaic_ms"], res["plots_annotate_ms"], res["plots_coefs_ms"] = (spread(stages[k]) for k in ("mosaic_ms", "annotate_ms", "coefs_ms"))
    res["plots_plot_batch_ms"], res["plots_plot_batch_timed_stages_ms"], res["plots_pillow_ms"] = spread(plain), spread(wall), spread(host)
    if opt.map:
        sweep = {}
        with tempfile.TemporaryDirectory() as tmp:
            for name, extra in (("warm_up", []), ("without", []), ("plots_3", ["--plots", "3"]), ("without_again", []), ("plots_3_again", ["--plots", "3"])):
                o = val.parse_opt(["--data", opt.map, "--weights", opt.weights, "--project", tmp, "--name", name, "--quiet", *extra])
                val.run(o, log=lambda *_: None)
                meta = json.load(open(os.path.join(tmp, name, "val.json")))
                sweep[name] = {"images_per_s": meta["images_per_s"], "images": meta["images"]}
        res["plots_sweep"] = sweep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.02)
    ap.add_argument("--detections", type=int, default=10_000_000)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--map", default=None, metavar="DATA.yaml")
    ap.add_argument("--weights", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--plots", action="store_true", help="only the --plots leg")
    opt = ap.parse_args()
    import numpy as np
    import torch
    from aquaculture_amd import engine, val
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(dev), "repeats": opt.repeats}
    if opt.plots:
        plots_leg(opt, res)
        print(json.dumps(res, indent=1))
        if opt.out:
            with open(opt.out, "w") as f:
                json.dump(res, f, indent=1)
        return

    # expand
    B, N, nc = 32, 25200, 5
    pred = rng.random((B, N, 5 + nc)).astype(np.float32)
    pred[..., 4] = np.where(rng.random((B, N)) < opt.share, 0.5, 0.0005)
    pred[..., 5:] = 0.5
    pred_d = torch.from_numpy(pred).to(dev)
    M = min(N * nc, engine.VAL_NMS_ROWS)
    rows = torch.empty((B, M, 5 + nc), dtype=torch.float32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(engine.load_library().aq_val_expand_scratch_bytes(B, N, nc), dtype=torch.uint8, device=dev)
    res["expand_ms"] = timed(lambda: engine.val_expand_rows(pred_d, 0.001, M, rows, counts, scratch), opt.repeats)
    res["expand"] = {"B": B, "N": N, "nc": nc, "share": opt.share, "rows_emitted_per_image": float(counts.float().mean())}

    # match
    Bm, D, L = 32, 300, 20
    lb = np.concatenate([rng.integers(0, 5, (Bm * L, 1)), rng.random((Bm * L, 2)) * 0.8 + 0.1, rng.random((Bm * L, 2)) * 0.1 + 0.02], 1).astype(np.float32)
    lbox = val.label_boxes(lb, 1024, 1024).reshape(Bm, L, 4)
    pick = rng.integers(0, L, (Bm, D))
    dets = np.zeros((Bm, D, 6), np.float32)
    geom = val.letterbox_geom((640, 640), (1024, 1024))
    dets[..., :4] = (np.take_along_axis(lbox, pick[..., None].repeat(4, 2), 1) + rng.normal(0, 4, (Bm, D, 4))) * geom[2]
    dets[..., 4] = np.sort(rng.random((Bm, D)), 1)[:, ::-1]
    dets[..., 5] = np.take_along_axis(lb[:, 0].reshape(Bm, L), pick, 1)
    dets_d, cnt_d = torch.from_numpy(dets).to(dev), torch.full((Bm,), D, dtype=torch.int32, device=dev)
    stats = val._DeviceStats(Bm * D, dev)
    boxes, classes, geoms = [lbox[b] for b in range(Bm)], [lb[:, 0].reshape(Bm, L)[b] for b in range(Bm)], np.tile(geom, (Bm, 1))
    start = np.arange(Bm + 1, dtype=np.int32) * L
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lbox_d, lcls_d, start_d, geom_d = up(lbox.reshape(-1, 4)), up(lb[:, 0].astype(np.int32)), up(start), up(geoms)
    sc = torch.empty(10 * Bm * L, dtype=torch.int32, device=dev)

    def match():
        stats.total.zero_()
        engine.val_match(dets_d, cnt_d, lbox_d, lcls_d, start_d, start, geom_d, val.IOUV, stats.conf, stats.cls, stats.bits, stats.total, sc)
    res["match_ms"] = timed(match, opt.repeats)
    res["match"] = {"B": Bm, "detections": D, "labels": L, "correct_at_0.5": int((stats.bits[:Bm * D] & 1).sum())}

    # confusion: the match step's inputs
    cm = torch.zeros((6, 6), dtype=torch.int64, device=dev)
    rows_c = torch.empty((Bm, 4), dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    sc_c = torch.empty(engine.load_library().aq_val_confusion_scratch_bytes(Bm, D, Bm * L), dtype=torch.uint8, device=dev)
    lcls_h = lb[:, 0].astype(np.int32)

    def confusion():
        engine.val_confusion(dets_d, cnt_d, lbox_d, lcls_d, start_d, start, geom_d, 5, val.CONFUSION_CONF, val.CONFUSION_IOU, cm, image=rows_c,
                             label_cls_host=lcls_h, flag=flag, scratch=sc_c)
    res["confusion_ms"] = timed(confusion, opt.repeats)
    cm.zero_()
    confusion()
    res["confusion"] = {"B": Bm, "detections": D, "labels": L, "classes": 5, "taking_part": int(rows_c[:, 1].sum()), "kept_pairs": int(rows_c[:, 2].sum()),
                        "kept_pairs_of_equal_classes": int(rows_c[:, 3].sum()), "matrix_sum": int(cm.sum()), "class_flag": int(flag.item())}

    # scores
    n = opt.detections
    conf = rng.random(n).astype(np.float32)
    cls = rng.integers(0, 5, n).astype(np.int32)
    bits = np.where(rng.random(n) < conf, (1 << np.minimum(rng.integers(0, 14, n), 10)) - 1, 0).astype(np.uint16)
    label_counts = np.full(5, n // 8, np.int64)
    conf_d, cls_d, bits_d = up(conf), up(cls), up(bits.view(np.int16))
    kernel = []

    def scores():
        t = {}
        out = val.score_gpu(conf_d, cls_d, bits_d, label_counts, times=t)
        kernel.append(t["scores_ms"])
        return out
    for _ in range(2):
        scores()
    kernel.clear()
    wall = []
    for _ in range(opt.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = scores()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["scores_kernels_ms"] = spread(kernel)
    res["scores_with_sort_and_copies_ms"] = spread(wall)
    res["scores"] = {"detections": n, "classes": 5, "scratch_bytes": int(engine.load_library().aq_val_scores_scratch_bytes(n, int(engine.val_score_runs(
        np.array([[0, n]]))[-1])))}
    if not opt.no_cpu:
        t0 = time.perf_counter()
        want = val.score_cpu(conf, cls, bits, label_counts)
        res["scores_numpy_ms"] = (time.perf_counter() - t0) * 1e3
        res["scores_same_bytes"] = all(g.tobytes() == w.tobytes() for g, w in zip(got[2:], want[2:]))

    # the per-precision table
    if opt.map:
        table = {}
        with tempfile.TemporaryDirectory() as tmp:
            for prec in ("fp32", "f16x3", "bf16", "fp8", "fp8w"):
                o = val.parse_opt(["--data", opt.map, "--weights", opt.weights, "--precision", prec, "--project", tmp, "--name", prec, "--quiet"])
                s = val.run(o, log=lambda *_: None)
                meta = json.load(open(os.path.join(tmp, prec, "val.json")))
                table[prec] = {"P": s["mp"], "R": s["mr"], "mAP50": s["map50"], "mAP50-95": s["map"], "images_per_s": meta["images_per_s"],
                               "images": meta["images"], "detections": meta["detections"]}
        res["precisions"] = table
    print(json.dumps(res, indent=1))
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
