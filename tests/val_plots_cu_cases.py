"""The mosaic kernel's cases for one value of AQ_NUM_CUS, run in a child process of tests/test_gpu_val_plots.py (the pattern of
tests/cu_cases.py): every case of tests/test_val_plots.py's MOSAIC_CASES and a mosaic of many rows, each compared with mosaic_numpy and
digested.  ``python tests/val_plots_cu_cases.py --out FILE`` writes {"num_cus_env", "cases": [{"id", "ok", "sha256", "units"}]}."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EXTRA = ((16, 24, 40, (70, 300)), (5, 17, 23, 1920))       # 280 rows x 2 chunks of 1024 pixels: several trips per workgroup at 13 CUs; a paste


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    out = ap.parse_args().out
    import torch
    from test_val_plots import MOSAIC_CASES, case_geometry, case_id, case_images
    from aquaculture_amd import engine, val_plots
    records = []
    try:
        for case in MOSAIC_CASES + EXTRA:
            geo = case_geometry(case)
            images = case_images(*case[:3])
            xtab, ytab = val_plots.mosaic_tables(geo)
            got = engine.val_mosaic(torch.from_numpy(images).cuda(), geo["n"], geo["ns"], geo["h"], geo["w"], xtab, ytab).cpu().numpy()
            records.append({"id": case_id(case), "ok": got.tobytes() == val_plots.mosaic_numpy(images, geo).tobytes(),
                            "sha256": hashlib.sha256(got.tobytes()).hexdigest(), "units": geo["size"][0] * ((geo["size"][1] + 1023) // 1024)})
        torch.cuda.synchronize()
    except RuntimeError as err:
        print(f"HIP error: {err}", file=sys.stderr)
        return 3
    with open(out, "w") as f:
        json.dump({"num_cus_env": os.environ.get("AQ_NUM_CUS"), "cases": records}, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
