"""Writes the two data fixtures of tests/test_overlaps.py from the reference's data directory:

  g15_wanted_bboxes.csv          the header and the rows of data/wanted_bboxes.csv (index, WKT polygon in EPSG:3857) whose rectangle strictly
                                 overlaps another row's (open interiors meet), in file order with their original indices, the text of every
                                 kept line unchanged.  A box's region depends only on the earlier boxes that overlap it, so this subset has
                                 the regions of the whole file.  The whole subset fits; no prefix is taken.
  g15_wanted_bboxes_dedup.json   the features of data/wanted_bboxes_dedup.csv (a GeoJSON despite its name: the reference's
                                 deduplicate_download_boxes output) for those indices, coordinates as json reads and writes them (doubles,
                                 shortest round-trip text)

Reads only those two data files.

    python tests/golden/make_overlaps_golden.py /path/to/reference/data
"""
import csv
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NUM = re.compile(r"-?\d+\.?\d*(?:[eE][-+]?\d+)?")


def main(src: str) -> int:
    with open(os.path.join(src, "wanted_bboxes.csv"), newline="") as f:
        rows = list(csv.reader(f))
    boxes = []
    for r in rows[1:]:
        v = [float(t) for t in NUM.findall(r[1])]
        boxes.append((min(v[0::2]), min(v[1::2]), max(v[0::2]), max(v[1::2])))
    order = sorted(range(len(boxes)), key=lambda k: boxes[k][0])
    keep = set()
    for p, i in enumerate(order):                           # sweep in x: only boxes whose x-ranges overlap are compared
        for j in order[p + 1:]:
            if boxes[j][0] >= boxes[i][2]:
                break
            if boxes[i][1] < boxes[j][3] and boxes[j][1] < boxes[i][3] and boxes[j][0] < boxes[i][2] and boxes[i][0] < boxes[j][2]:
                keep.update((i, j))
    with open(os.path.join(HERE, "g15_wanted_bboxes.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(rows[0])
        for k in sorted(keep):
            w.writerow(rows[1 + k])
    ids = {int(rows[1 + k][0]) for k in keep}
    with open(os.path.join(src, "wanted_bboxes_dedup.csv")) as f:
        doc = json.load(f)
    feats = [{"type": "Feature", "properties": {"bbox_ind": int(ft["properties"]["bbox_ind"])}, "geometry": ft["geometry"]}
             for ft in doc["features"] if int(ft["properties"]["bbox_ind"]) in ids]
    with open(os.path.join(HERE, "g15_wanted_bboxes_dedup.json"), "w") as f:
        json.dump({"type": "FeatureCollection", "crs": doc.get("crs"), "features": feats}, f, separators=(",", ":"))
    print(f"{len(keep)} of {len(boxes)} boxes overlap another; {len(feats)} of them have a region in the shipped file")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
