"""Writes the two data fixtures of tests/test_kfold.py from the reference's data directory:

  g14_known_sites.csv       the rows of data/aquaculture_med_dedupe.csv (id, lat, lon, num_cages) whose site lies between 2 and 10 degrees east
                            and 41 and 44.5 degrees north -- the French coast and Corsica, where the scenes of g12 are --, the text of every
                            kept line unchanged
  g14_wanted_bboxes.csv     the header and the rows 1956 and 1962 of data/wanted_bboxes.csv (index, WKT polygon in EPSG:3857): the two scenes
                            the labels of g12_humanlabels_1956_1962.json were cut from, so that their images have rectangles

    python tests/golden/make_kfold_golden.py /path/to/reference/data
"""
import csv
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ("1956", "1962")
LON, LAT = (2.0, 10.0), (41.0, 44.5)


def main(src: str) -> int:
    with open(os.path.join(src, "aquaculture_med_dedupe.csv")) as f:
        lines = f.read().splitlines()
    header = lines[0].split(",")
    a, o = header.index("lat"), header.index("lon")
    keep = [l for l in lines[1:] if l.strip() and LAT[0] <= float(l.split(",")[a]) <= LAT[1] and LON[0] <= float(l.split(",")[o]) <= LON[1]]
    with open(os.path.join(HERE, "g14_known_sites.csv"), "w") as f:
        f.write("\n".join([lines[0]] + keep) + "\n")
    with open(os.path.join(src, "wanted_bboxes.csv"), newline="") as f:
        rows = list(csv.reader(f))
    with open(os.path.join(HERE, "g14_wanted_bboxes.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(rows[0])
        for r in rows[1:]:
            if r[0] in SCENES:
                w.writerow(r)
    print(f"{len(keep)} of {len(lines) - 1} sites, {len(SCENES)} scenes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
