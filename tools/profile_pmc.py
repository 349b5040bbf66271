#!/usr/bin/env python3
"""Per-op hardware counters for the bench workload (runs ON the GPU box).

Runs `bench.py` under `rocprofv3 --pmc` once per counter group (counters in their own passes, with
kernel-trace only -- never with sys/hip/hsa tracing), maps every kernel dispatch of the timed steps back to its
plan op by KERNEL NAME in plan order (a step starts with the stem kernel; every op kind has its kernel families, auxiliary
dispatches -- the fused heads' counter memset and gather -- go to the op they serve; round 2 mapped by position and mislabelled the
head rows once the heads were fused; the engine's roctx ranges cannot help here: counter passes must not enable marker tracing) and
writes a per-op table.  FETCH_SIZE is doubled as /opt/skills/guides/MI355X_MICROARCH.md (HBM section) prescribes for
gfx950 wide coalesced reads; WRITE_SIZE is taken as is; both are in KiB in rocprofv3's output.

    python tools/profile_pmc.py --out gpurun_out/pmc_r01 [--batch 64] [--groups sq1 sq2 fetch write]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {
    "sq1": "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE",
    "sq2": "SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_VMEM SQ_INSTS_SALU SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_VMEM",
    "fetch": "FETCH_SIZE",
    "write": "WRITE_SIZE",
    "l2": "TCC_HIT_sum TCC_MISS_sum",
}


def run_pass(name, counters, out, batch, steps):
    d = os.path.join(out, name)
    os.makedirs(d, exist_ok=True)
    env = dict(os.environ, TMPDIR="/tmp", AQ_TUNE_CACHE=os.path.join(out, "tune_cache.json"))
    cmd = ["rocprofv3", "--kernel-trace", "--pmc", *counters.split(), "--output-format", "csv", "-d", d, "-o", "pmc", "--",
           sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1", "--batch", str(batch),
           "--no-cpu-baseline", "--no-profile", "--parity-steps", "0"]
    r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True)
    with open(os.path.join(d, "log.txt"), "w") as f:
        f.write(r.stdout[-4000:] + "\n---\n" + r.stderr[-4000:])
    if r.returncode != 0:
        print(f"pass {name} failed rc={r.returncode}: {r.stderr[-600:]}", file=sys.stderr)
        return None
    files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    return files[0] if files else None


def run_stats(out, batch):
    """`rocprofv3 --kernel-trace --stats` of the default bench command; returns (bench json, 3x3 avg launch us)."""
    d = os.path.join(out, "stats")
    os.makedirs(d, exist_ok=True)
    env = dict(os.environ, TMPDIR="/tmp", AQ_TUNE_CACHE=os.path.join(out, "tune_cache.json"))
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "bench", "--",
           sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "3", "--batch", str(batch), "--no-cpu-baseline", "--parity-steps", "0"]
    r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True)
    with open(os.path.join(d, "bench_stdout.json"), "w") as f:
        f.write(r.stdout)
    if r.returncode != 0:
        print("stats pass failed:", r.stderr[-500:], file=sys.stderr)
    return d


def parse(path):
    """-> list of dispatches in order: {name, counters{}, dur_ns}"""
    by_id = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            did = int(row["Dispatch_Id"])
            d = by_id.setdefault(did, {"name": row["Kernel_Name"], "c": {}, "vgpr": row.get("VGPR_Count"), "lds": row.get("LDS_Block_Size"),
                                       "grid": row.get("Grid_Size"), "wg": row.get("Workgroup_Size"),
                                       "dur": int(row.get("End_Timestamp", 0) or 0) - int(row.get("Start_Timestamp", 0) or 0)})
            d["c"][row["Counter_Name"]] = d["c"].get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    return [by_id[k] for k in sorted(by_id)]


FIRST_KERNELS = ("stem_conv_kernel", "preprocess_s2d_kernel")   # the kernel a step starts with (fused stem / two-kernel stem)


PLAN = [None]


def op_patterns(o, spec):
    """Kernel-name fragments an op of the plan may launch."""
    if o.kind == spec.OP_STEM:
        return ("stem_conv_kernel",)
    if o.kind == spec.OP_PREPROCESS:
        return ("preprocess_s2d_kernel",)
    if o.kind == spec.OP_DOWNBLOCK:
        return ("downblock_kernel",)
    if o.kind == spec.OP_BOTTLENECK:
        return ("bottleneck_kernel", "bottleneck_asm")
    if o.kind == spec.OP_SPPF_POOL:
        return ("sppf_pool",)
    if o.kind == spec.OP_UPSAMPLE2X:
        return ("upsample2x_kernel",)
    if o.kind == spec.OP_DECODE:
        return ("decode_kernel",)
    if o.kind == spec.OP_NMS:
        return ("nms_kernel",)
    if o.level >= 0:
        return ("head_decode_kernel", "conv_igemm_kernel")
    return ("conv_igemm_kernel", "conv3x3_halo_kernel", "conv1x1_direct_kernel", "conv1x1_asm", "conv3x3_pl", "downblock_kernel")


def steps_of(disp, kernels_per_step=None):
    """-> list of steps; a step = list of (op index, dispatch), dispatches matched to plan ops by kernel name in plan order.  A dispatch no
    later op claims (memset / counter gather of the fused heads) is booked on the op before it; an op without a dispatch (the decode op of
    the fused-head path) simply gets none.  Steps whose kernel sequence does not walk the whole plan are dropped."""
    from aquaculture_amd import spec
    plan = PLAN[0]
    pats = [op_patterns(o, spec) for o in plan.ops]
    starts = [i for i, d in enumerate(disp) if any(k in d["name"] for k in FIRST_KERNELS)] + [len(disp)]
    out = []
    for a_, b_ in zip(starts[:-1], starts[1:]):
        cur, step, ok = 0, [], True
        for d in disp[a_:b_]:
            nxt = next((j for j in range(cur, len(pats)) if any(p_ in d["name"] for p_ in pats[j])), None)
            # an auxiliary kernel matches nothing ahead -- or only something implausibly far ahead (more than the few ops a fused path skips)
            if nxt is None or nxt > cur + 3:
                step.append((max(cur - 1, 0), d))
                continue
            step.append((nxt, d))
            cur = nxt + (2 if "bottleneck_asm_c48_tail" in d["name"] else 1)      # (the C3 tail computes the next op, cv3, too)
        seen = {i for i, _ in step}
        seen |= {i + 1 for i, d in step if "bottleneck_asm_c48_tail" in d["name"]}     # the C3 tail: cv3 runs inside the Bottleneck's launch
        need = {i for i, o in enumerate(plan.ops) if o.kind != spec.OP_DECODE}
        if need - seen:
            ok = False
        if ok:
            out.append(step)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "pmc"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--groups", nargs="+", default=["stats", "sq1", "sq2", "fetch", "write"])
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)
    os.makedirs(a.out, exist_ok=True)
    # tuned configs first (outside any profiler), so the profiled runs launch no tuning kernels
    env = dict(os.environ, AQ_TUNE_CACHE=os.path.join(a.out, "tune_cache.json"))
    subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", str(a.batch),
                    "--no-cpu-baseline"], env=env, capture_output=True, text=True, check=True)
    sys.path.insert(0, ROOT)
    from aquaculture_amd import spec
    plan = spec.build_plan("yolov5m", 5, fused_bottleneck=True)   # what a bf16 Engine (and bench.py) runs
    fl = plan.flops(640, 640)
    PLAN[0] = plan
    if "stats" in a.groups:
        a.groups = [g for g in a.groups if g != "stats"]
        sd = run_stats(a.out, a.batch)
        tr = glob.glob(os.path.join(sd, "**", "*kernel_trace.csv"), recursive=True)
        if tr:
            disp = []
            with open(tr[0]) as f:
                for row in csv.DictReader(f):
                    disp.append({"name": row["Kernel_Name"], "dur": int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), "start": int(row["Start_Timestamp"])})
            disp.sort(key=lambda d: d["start"])
            st = steps_of(disp)[-10:]                    # the 10 single-stream steps of bench.py's roofline pass (the last ones)
            idx3 = [i for i, o in enumerate(plan.ops) if o.kind == spec.OP_CONV and o.meta.get("class") == "conv3x3"]
            durs = [d["dur"] for step in st for op_, d in step if op_ in idx3]
            idx_all3 = set(idx3) | {i for i, o in enumerate(plan.ops) if o.kind in (spec.OP_BOTTLENECK, spec.OP_DOWNBLOCK)}
            d_all3 = sum(d["dur"] for step in st for op_, d in step if op_ in idx_all3) / max(len(st), 1)
            f_all3 = sum(plan.ops[i].flops_per_tile for i in idx_all3) * a.batch
            by_kernel = defaultdict(lambda: [0, 0])
            for step in st:
                for op_, d in step:
                    if op_ in idx3:
                        k_ = d["name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0][:48]
                        by_kernel[k_][0] += 1
                        by_kernel[k_][1] += d["dur"]
            summ = {"steps": len(st), "which": "last 10 steps of the run = bench.py's single-stream roofline pass", "conv3x3_launches": len(durs), "conv3x3_avg_launch_us": sum(durs) / max(len(durs), 1) / 1e3,
                    "conv3x3_ms_per_step": sum(durs) / max(len(st), 1) / 1e6,
                    "conv3x3_tflops": sum(plan.ops[i].flops_per_tile for i in idx3) * a.batch / (sum(durs) / max(len(st), 1)) / 1e3,
                    "conv3x3_by_kernel_avg_us": {k_: round(v_[1] / v_[0] / 1e3, 2) for k_, v_ in sorted(by_kernel.items())},
                    "all_3x3_kernels_ms_per_step": d_all3 / 1e6, "all_3x3_tflops": f_all3 / max(d_all3, 1) / 1e3,
                    "all_kernels_ms_per_step": sum(d["dur"] for step in st for _, d in step) / max(len(st), 1) / 1e6}
            with open(os.path.join(a.out, "stats_summary.json"), "w") as f:
                json.dump(summ, f, indent=1)
            print("kernel-trace summary:", json.dumps(summ))
    merged = defaultdict(lambda: defaultdict(float))
    meta = {}
    for g in a.groups:
        path = run_pass(g, GROUPS[g], a.out, a.batch, a.steps)
        if not path:
            continue
        st = steps_of(parse(path))
        st = st[1:] if len(st) > 1 else st          # drop the warm-up step when there is another
        for step in st:
            for op, d in step:
                for k, v in d["c"].items():
                    merged[op][k] += v / len(st)
                merged[op]["dur_ns_" + g] += d["dur"] / len(st)
                if op not in meta or any(p_ in d["name"] for p_ in op_patterns(plan.ops[op], spec)):
                    meta[op] = (d["name"], d["vgpr"], d["lds"], d["grid"], d["wg"])
    rows = []
    for i, o in enumerate(plan.ops):
        c = merged.get(i, {})
        rows.append({"op": i, "name": o.name, "kernel": meta.get(i, ("",))[0][:80], "vgpr": meta.get(i, ("", "", "", "", ""))[1],
                     "lds": meta.get(i, ("", "", "", "", ""))[2], "grid": meta.get(i, ("", "", "", "", ""))[3],
                     "flops": o.flops_per_tile * a.batch, **{k: v for k, v in c.items()}})
    with open(os.path.join(a.out, "per_op.json"), "w") as f:
        json.dump({"batch": a.batch, "rows": rows}, f)
    # HBM traffic per launch of the dominant kernel (the 3x3 conv launches), gfx950 correction applied
    r3 = [r for r, o in zip(rows, plan.ops) if o.kind == spec.OP_CONV and o.meta.get("class") == "conv3x3" and "FETCH_SIZE" in r and "WRITE_SIZE" in r]
    if r3:
        rd = sum(2 * r["FETCH_SIZE"] * 1024 for r in r3) / len(r3)
        wr = sum(r["WRITE_SIZE"] * 1024 for r in r3) / len(r3)
        with open(os.path.join(a.out, "hbm_traffic.json"), "w") as f:
            lib_digest = ""
            try:
                lib_digest = open(os.path.join(ROOT, "aquaculture_amd", "csrc", "libaqengine.so.sha256")).read().strip()
            except OSError:
                pass
            cfgs = {}
            try:
                tc = json.load(open(os.path.join(a.out, "tune_cache.json")))
                cfgs = {k: [v[i] for i, o in enumerate(plan.ops) if o.kind == spec.OP_CONV and o.meta.get("class") == "conv3x3"] for k, v in tc.items()}
            except (OSError, ValueError):
                pass
            if not cfgs:
                # the shipped table answered the tuner (no cache file is written then): record ITS picks for this geometry, so that bench.py's
                # "same tuned 3x3 kernels" is a comparison, not an assumption
                try:
                    ship = json.load(open(os.path.join(ROOT, "aquaculture_amd", "data", "tuned_tables.json")))
                    cfgs = {k: [v[i] for i, o in enumerate(plan.ops) if o.kind == spec.OP_CONV and o.meta.get("class") == "conv3x3"]
                            for k, v in ship.items() if f":pbf16:{a.batch}x640x640:" in k and k.startswith("yolov5m:") and len(v) == len(plan.ops)}
                except (OSError, ValueError):
                    pass
            json.dump({"kernel": f"conv3x3_pl_asm_pm13w40 / pm13w20 (nb13) / conv3x3_pl_asm_s2nb13 / downblock_kernel / conv_igemm_kernel on the {len(r3)} 3x3 layers launched as plain convs", "batch": a.batch, "launches_averaged": len(r3),
                       "library_source_digest": lib_digest, "conv3x3_configs": cfgs,
                       "read_bytes_per_launch": rd, "write_bytes_per_launch": wr, "bytes_per_launch": rd + wr,
                       "method": "rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate passes; FETCH_SIZE x2 (gfx950 counts 128-B "
                                 "requests at 64 B, MI355X_MICROARCH.md HBM section), KiB -> bytes; mean over these launches of one step"}, f, indent=1)
    # compact text table
    def g(r, k):
        return r.get(k, 0.0)
    lines = ["op name                     us     TF/s  mfma%  valu%  lds%  wait%  waitinst% | VALU/MFMA inst  ldsconf% | rdMB  wrMB   HBM TB/s"]
    for r in rows:
        dur = g(r, "dur_ns_sq1") or g(r, "dur_ns_sq2") or g(r, "dur_ns_fetch")
        if not dur:
            continue
        wc = g(r, "SQ_WAVE_CYCLES") or 1.0
        busy = g(r, "SQ_BUSY_CYCLES") or 1.0
        mf = g(r, "SQ_INSTS_MFMA") or 0.0
        line = "%3d %-22s %7.1f %7.1f %6.1f %6.1f %5.1f %6.1f %9.1f | %7.1f %8.0f %7.1f | %6.1f %6.1f %8.2f" % (
            r["op"], r["name"][:22], dur / 1e3, r["flops"] / max(dur, 1) / 1e3,
            100 * g(r, "SQ_VALU_MFMA_BUSY_CYCLES") / (busy * 4 if busy else 1),
            100 * g(r, "SQ_ACTIVE_INST_VALU") / wc, 100 * g(r, "SQ_ACTIVE_INST_LDS") / wc, 100 * g(r, "SQ_WAIT_ANY") / wc,
            100 * g(r, "SQ_WAIT_INST_ANY") / wc,
            g(r, "SQ_INSTS_VALU") / mf if mf else 0.0, mf,
            100 * g(r, "SQ_LDS_BANK_CONFLICT") / max(g(r, "SQ_LDS_IDX_ACTIVE"), 1.0),
            2 * g(r, "FETCH_SIZE") / 1024, g(r, "WRITE_SIZE") / 1024,
            (2 * g(r, "FETCH_SIZE") + g(r, "WRITE_SIZE")) * 1024 / max(dur, 1) / 1e3)   # bytes / ns = GB/s; / 1e3 = TB/s
        lines.append(line)
    txt = "\n".join(lines)
    with open(os.path.join(a.out, "per_op.txt"), "w") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
