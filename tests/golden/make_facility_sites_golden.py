"""Writes the three data fixtures of tests/test_facility_sites.py from the reference tree:

  g16_label_boxes.npz       the bounds (float64 [n, 4]: x0, y0, x1, y1 in EPSG:3857), the year (int16 [n]) and the type (uint8 [n], an index into
                            ``types``) of every feature of output/humanlabels.geojson, in file order; compressed numpy arrays, so that
                            the 4142 x 4 doubles stay exact and the file stays small (a JSON of them is 0.4 MB of digits)
  g16_known_sites.csv       the columns lat, lon, num_cages of data/aquaculture_med_dedupe.csv, the text of every field unchanged
  g16_wanted_bboxes.csv     the header and those rows of data/wanted_bboxes.csv (index, WKT polygon in EPSG:3857) that reach the table's total
                            bounds on one of the four sides, the text of every kept line unchanged: the total bounds of this subset are
                            those of the whole file, which is all the step needs of it

    python tests/golden/make_facility_sites_golden.py /path/to/reference
"""
import csv
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
COLUMNS = ("lat", "lon", "num_cages")


def main(src: str) -> int:
    with open(os.path.join(src, "output", "humanlabels.geojson")) as f:
        obj = json.load(f)
    bounds, years, types = [], [], []
    for feat in obj["features"]:
        assert feat["geometry"]["type"] == "Polygon"
        ring = feat["geometry"]["coordinates"][0]
        xs, ys = [float(p[0]) for p in ring], [float(p[1]) for p in ring]
        bounds.append([min(xs), min(ys), max(xs), max(ys)])
        years.append(int(feat["properties"]["year"]))
        types.append(str(feat["properties"]["type"]))
    import numpy as np
    names = sorted(set(types))
    np.savez_compressed(os.path.join(HERE, "g16_label_boxes.npz"), bounds=np.asarray(bounds, np.float64), year=np.asarray(years, np.int16),
                        type=np.asarray([names.index(t) for t in types], np.uint8), types=np.asarray(names))
    with open(os.path.join(src, "data", "aquaculture_med_dedupe.csv"), newline="") as f:
        rows = list(csv.reader(f))
    at = [rows[0].index(c) for c in COLUMNS]
    with open(os.path.join(HERE, "g16_known_sites.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(COLUMNS)
        for r in rows[1:]:
            if r:
                w.writerow([r[i] for i in at])
    with open(os.path.join(src, "data", "wanted_bboxes.csv"), newline="") as f:
        boxes = list(csv.reader(f))
    g = boxes[0].index("geometry")
    rect = []
    for r in boxes[1:]:
        nums = [float(v) for v in re.findall(r"-?\d+\.?\d*(?:[eE][-+]?\d+)?", r[g])]
        rect.append((min(nums[0::2]), min(nums[1::2]), max(nums[0::2]), max(nums[1::2])))
    total = (min(b[0] for b in rect), min(b[1] for b in rect), max(b[2] for b in rect), max(b[3] for b in rect))
    with open(os.path.join(HERE, "g16_wanted_bboxes.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(boxes[0])
        kept = 0
        for r, b in zip(boxes[1:], rect):
            if any(b[i] == total[i] for i in range(4)):
                w.writerow(r)
                kept += 1
    print(f"{len(bounds)} labels, {len(rows) - 1} sites, {kept} of {len(rect)} boxes reach the total bounds {total}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
