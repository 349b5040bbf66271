"""Writes tests/golden/g13_model_error_labels.json: the human labels of the 42 images of g12_humanlabels_1956_1962.json (the features of
the reference's output/humanlabels.geojson whose image belongs to scene 1956 or 1962, in the file's order, so row for row the labels of
g12) with the six columns the label areas need beside g12's: the label's box in the pixels of its image (xmin, ymin, xmax, ymax) and that
image's size (jpeg_width, jpeg_height).  Data only, as compact JSON by column, the doubles unchanged; ``image`` indexes ``images``.
tests/test_model_errors.py turns it back into a GeoJSON FeatureCollection.

    python tests/golden/make_model_errors_golden.py /path/to/reference/output/humanlabels.geojson
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
G12 = os.path.join(HERE, "g12_humanlabels_1956_1962.json")
OUT = os.path.join(HERE, "g13_model_error_labels.json")
PIXEL_COLUMNS = ("xmin", "ymin", "xmax", "ymax", "jpeg_width", "jpeg_height")


def main(src: str) -> int:
    with open(G12) as f:
        g12 = json.load(f)
    with open(src) as f:
        obj = json.load(f)
    wanted = set(g12["images"])
    feats = [ft for ft in obj["features"] if ft["properties"]["image"] in wanted]
    bounds = []
    for ft in feats:
        ring = ft["geometry"]["coordinates"][0]
        xs, ys = sorted({p[0] for p in ring}), sorted({p[1] for p in ring})
        assert len(ring) == 5 and len(xs) == 2 and len(ys) == 2, ring
        bounds.append([xs[0], ys[0], xs[1], ys[1]])
    images = sorted({ft["properties"]["image"] for ft in feats})
    out = {"crs": obj["crs"], "images": images, "image": [images.index(ft["properties"]["image"]) for ft in feats],
           "type": [ft["properties"]["type"] for ft in feats], "year": [ft["properties"]["year"] for ft in feats], "bounds": bounds}
    out.update({c: [ft["properties"][c] for ft in feats] for c in PIXEL_COLUMNS})
    assert images == g12["images"] and bounds == g12["bounds"] and out["type"] == g12["type"] and out["year"] == g12["year"], "not the labels of g12"
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"{len(feats)} labels of {len(images)} images, {os.path.getsize(OUT)} bytes in {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
