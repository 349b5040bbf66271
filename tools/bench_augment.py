"""Plain vs augmented (--augment) throughput of the engine, one process, steps alternating.

Setup: yolov5m bf16 (BASELINE.json configs[1]'s model and precision), batch 64, resident synthetic 640-px tiles, seeded synthetic weights,
tuned tables for all three geometries an augmented call runs at (640, 544, 448; Engine.autotune(augment=True), from the caches where
present).  Timing: after a warm-up, windows of plain and augmented steps alternate; each window runs steps back to back for at least
--window seconds between two device events.  Prints one JSON line: tiles/s of both (median over windows), their ratio, and per pass the
kernel family of every conv op (aq_engine_last_launch_augment).

    python tools/bench_augment.py [--batch 64] [--windows 6] [--window 2.0]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--windows", type=int, default=6, help="windows per mode (alternating)")
    ap.add_argument("--window", type=float, default=2.0, help="minimum seconds per window")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch
    from aquaculture_amd import augment, checkpoint, tiles
    from aquaculture_amd.build import build
    from aquaculture_amd.engine import Engine
    build()
    ck = checkpoint.synthetic_checkpoint("yolov5m", 5)
    eng = Engine(ck, args.precision)
    x = torch.from_numpy(tiles.synthetic_batch([i % 64 for i in range(args.batch)], args.size)).cuda()
    tables = eng.autotune(x, augment=True, cache=os.environ.get("AQ_TUNE_CACHE"))
    B = args.batch
    for _ in range(args.warmup):
        eng.infer(x)
        eng.infer(x, augment=True)
    torch.cuda.synchronize()

    def window(aug):
        # steps per window sized from one timed step so that the window lasts at least args.window seconds
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.infer(x, augment=aug)
        e1.record()
        e1.synchronize()
        n = max(3, int(args.window * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
        e0.record()
        for _ in range(n):
            eng.infer(x, augment=aug)
        e1.record()
        e1.synchronize()
        return n * B / (e0.elapsed_time(e1) / 1e3)

    rates = {False: [], True: []}
    for _ in range(args.windows):
        for aug in (False, True):
            rates[aug].append(window(aug))
    plain, aug = statistics.median(rates[False]), statistics.median(rates[True])
    eng.infer(x, augment=True)
    torch.cuda.synchronize()
    passes, n_aug = augment.geometry(args.size, args.size, ck.na)
    conv = [i for i, o in enumerate(eng.plan.ops) if o.kind == 1]
    per_pass = []
    for p, ps in enumerate(passes):
        fam = eng.last_launches(augment_pass=p)
        per_pass.append({"geometry": [B, ps.hp, ps.wp], "families": {eng.plan.ops[i].name: f"{fam[i][0]}:{fam[i][1]}" for i in conv}})
    print(json.dumps({"model": "yolov5m", "precision": args.precision, "batch": B, "size": args.size, "rows_per_image": n_aug,
                      "plain_tiles_per_s": round(plain, 1), "augment_tiles_per_s": round(aug, 1), "plain_over_augment": round(plain / aug, 3),
                      "windows": {"plain": [round(r, 1) for r in rates[False]], "augment": [round(r, 1) for r in rates[True]]},
                      "tuned_geometries": [list(g) for g, _ in tables], "passes": per_pass}))


if __name__ == "__main__":
    main()
