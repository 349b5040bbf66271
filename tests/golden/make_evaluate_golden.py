"""Writes tests/golden/g12_humanlabels_1956_1962.json: the human labels of two scenes of the reference's output/humanlabels.geojson (the
features whose image belongs to scene 1956 or 1962), their properties cut to image, type and year.  Data only, as compact JSON by column:
every label of the file is an axis-aligned rectangle (checked here), so its ring is kept as its bounds [xmin, ymin, xmax, ymax], the
doubles unchanged; ``image`` indexes ``images``.  tests/test_evaluate.py turns it back into a GeoJSON FeatureCollection.

    python tests/golden/make_evaluate_golden.py /path/to/reference/output/humanlabels.geojson
"""
import json
import os
import sys

SCENES = ("1956", "1962")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g12_humanlabels_1956_1962.json")


def scene_of(image: str) -> str:
    """ORTHOIMAGERY.ORTHOPHOTOS<year>_<scene>_<x>_<y>.jpeg -> <scene>"""
    return image.split("_")[1]


def main(src: str) -> int:
    with open(src) as f:
        obj = json.load(f)
    feats = [ft for ft in obj["features"] if scene_of(ft["properties"]["image"]) in SCENES]
    images = sorted({ft["properties"]["image"] for ft in feats})
    bounds = []
    for ft in feats:
        assert ft["geometry"]["type"] == "Polygon" and len(ft["geometry"]["coordinates"]) == 1
        ring = ft["geometry"]["coordinates"][0]
        xs, ys = sorted({p[0] for p in ring}), sorted({p[1] for p in ring})
        assert len(ring) == 5 and ring[0] == ring[4] and len(xs) == 2 and len(ys) == 2, ring
        assert {(p[0], p[1]) for p in ring} == {(x, y) for x in xs for y in ys}, ring
        bounds.append([xs[0], ys[0], xs[1], ys[1]])
    out = {"crs": obj["crs"], "images": images, "image": [images.index(ft["properties"]["image"]) for ft in feats],
           "type": [ft["properties"]["type"] for ft in feats], "year": [ft["properties"]["year"] for ft in feats], "bounds": bounds}
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"{len(feats)} labels, {os.path.getsize(OUT)} bytes in {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
