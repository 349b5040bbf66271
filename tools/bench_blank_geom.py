#!/usr/bin/env python3
"""What --blank-geom costs.

  kernel   aq_blank_components_u8 and aq_blank_ring_edges_u8 on a batch of 64 tiles of 1024 px in HBM of which 0, 8 or 64 qualify (partly blank
           by the records of aq_blank_stats_u8, which are given to the call): HIP events around `calls` calls after warm-up, `repeats` times,
           microseconds per call as median and range; aq_blank_stats_u8 on the same batch beside it.  With 0 qualifying frames every workgroup
           leaves after reading its frame's record: the skip path.
  sweep    detect.py over a directory of synthetic 1024-px JPEG tiles, `--white` of them with a white margin, with --blank-key and with
           --blank-geom, interleaved, `--runs` each: the steady-state images/s each run prints.  With --white 0 no tile is partly blank and
           the --blank-geom run launches nothing the --blank-key run does not.

    python tools/bench_blank_geom.py [--tiles 1024] [--white 128] [--runs 2] [--skip-sweep] [--out result.json]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_times(batch=64, size=1024, calls=20, repeats=5):
    import numpy as np
    import torch
    from aquaculture_amd.engine import (blank_components, blank_frame_table, blank_geom_frame_table, blank_stats, load_library)
    lib = load_library()
    rows = []
    for qualifying in (0, 8, 64):
        g = torch.Generator(device="cuda").manual_seed(1)
        tiles = torch.randint(0, 240, (batch, size, size, 3), generator=g, device="cuda", dtype=torch.uint8)
        tiles[:qualifying, :, size - 100:] = 255            # a white margin: partly blank; the non-blank part is one region of 924 columns
        tiles[:qualifying, 200:260, 300:420] = 255          # with a lake
        stats = blank_stats(tiles.view(-1), blank_frame_table(np.arange(batch, dtype=np.int64) * size * size * 3, size * 3, [(size, size)] * batch)).contiguous()
        table = blank_geom_frame_table(np.arange(batch, dtype=np.int64) * size * size * 3, size * 3, [(size, size)] * batch)
        scratch = torch.empty(int(lib.aq_blank_geom_scratch_bytes(table.ctypes.data, batch)), dtype=torch.uint8, device="cuda")
        out = torch.empty((batch, 12), dtype=torch.int32, device="cuda")
        table_dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
        rec = blank_components(tiles.view(-1), table, stats_dev=stats, scratch=scratch, out=out, frames_dev=table_dev)[0].cpu().numpy()
        assert int(rec[:, 0].sum()) == qualifying
        at = np.zeros(batch + 1, np.int64)
        at[1:] = np.cumsum(rec[:, 10])
        at_dev = torch.from_numpy(at).cuda()
        edges = torch.empty((max(int(at[-1]), 1), 2), dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def components():
            blank_components(tiles.view(-1), table, stats_dev=stats, scratch=scratch, out=out, frames_dev=table_dev)

        def ring_edges():
            rc = lib.aq_blank_ring_edges_u8(table_dev.data_ptr(), table.ctypes.data, batch, scratch.data_ptr(), scratch.numel(), out.data_ptr(),
                                            at_dev.data_ptr(), at.ctypes.data, edges.data_ptr(), edges.shape[0], stream)
            assert rc == 0

        def timed(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            got = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                got.append(e0.elapsed_time(e1) * 1e3 / calls)  # microseconds per call
            return {"median_us": round(statistics.median(got), 1), "min_us": round(min(got), 1), "max_us": round(max(got), 1)}

        rows.append({"qualifying": qualifying, "components": timed(components), "ring_edges": timed(ring_edges), "edge_px": int(at[-1])})
    return {"batch": batch, "tile": size, "calls": calls, "repeats": repeats, "rows": rows}


def sweep_rates(n_tiles, n_white, runs, batch=64):
    import numpy as np
    from PIL import Image
    from aquaculture_amd import checkpoint, tiles
    rates = {"blank_key": [], "blank_geom": []}
    with tempfile.TemporaryDirectory() as d:
        tiles.write_synthetic_jpegs(os.path.join(d, "jpegs"), list(range(n_tiles)), size=1024)
        names = sorted(os.listdir(os.path.join(d, "jpegs")))
        for name in names[::max(1, n_tiles // n_white)][:n_white] if n_white else ():
            path = os.path.join(d, "jpegs", name)
            im = np.asarray(Image.open(path)).copy()
            im[:, 900:] = 255
            Image.fromarray(im).save(path, quality=95)
        checkpoint.write_synthetic_checkpoint(os.path.join(d, "w.pt"), "yolov5m", 5)
        for r in range(runs):
            for kind in ("blank_key", "blank_geom"):
                cmd = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", os.path.join(d, "w.pt"), "--source",
                       os.path.join(d, "jpegs"), "--save-txt", "--save-conf", "--nosave", "--quiet", "--half", "--project", os.path.join(d, "runs"),
                       "--name", f"{kind}{r}", "--batch-size", str(batch), "--autotune", "off", "--" + kind.replace("_", "-")]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    raise RuntimeError(p.stdout[-2000:] + p.stderr[-2000:])
                m = re.search(r"steady state: ([0-9.]+) images/s", p.stdout)
                rates[kind].append(float(m.group(1)) if m else None)
    return {"tiles": n_tiles, "white": n_white, "batch": batch, "steady_images_per_s": rates}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--white", type=int, default=128)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_blank_geom needs a GPU: there is nothing to measure without one")
    res = {"kernel": kernel_times()}
    print(json.dumps(res["kernel"]), flush=True)
    if not a.skip_sweep:
        res["sweep"] = sweep_rates(a.tiles, a.white, a.runs)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
