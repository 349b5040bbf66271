#!/usr/bin/env python3
"""Generates tests/golden/g10_blank_key.json: the status the reference's own ``is_blank`` / ``is_partly_blank`` (reference src/utils.py) give
seeded images and the decoded pixels of small JPEG files.  The two functions are loaded out of the reference's file when this script runs
(their definitions are compiled from its syntax tree; the module itself imports packages that are not needed for them); none of their text is
kept, only the recorded results: seed, shape, SHA-256 of the pixel bytes, status.
Run from the repo root: python tests/golden/make_blank_golden.py <reference checkout>/src/utils.py"""
import ast
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "g10_blank_key.json")

# (kind, h, w): what build_image makes of a seed
CASES = [("noise", 64, 64), ("noise", 7, 13), ("noise", 1, 1), ("dark", 96, 80), ("near_white", 64, 48), ("white", 32, 32), ("black", 16, 24),
         ("ones", 8, 8), ("twos", 8, 8), ("white_row", 40, 56), ("white_col", 56, 40), ("white_margin", 128, 96), ("one_channel", 32, 32),
         ("near_white_dark_px", 48, 48), ("jpeg_noise", 64, 64), ("jpeg_white_margin", 96, 128), ("jpeg_white", 48, 48), ("jpeg_dark", 80, 64)]


def build_image(kind: str, h: int, w: int, seed: int) -> np.ndarray:
    """The case's uint8 RGB image [h, w, 3]; the jpeg_* kinds go through a quality-95 JPEG file and back (Pillow)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = kind[5:] if kind.startswith("jpeg_") else kind
    if base == "noise":
        img = rng.integers(0, 256, (h, w, 3))
    elif base == "dark":
        img = rng.integers(0, 120, (h, w, 3))
    elif base == "near_white":
        img = rng.integers(250, 256, (h, w, 3))
    elif base in ("white", "black", "ones", "twos"):
        img = np.full((h, w, 3), {"white": 255, "black": 0, "ones": 1, "twos": 2}[base])
    elif base == "white_row":
        img = rng.integers(0, 100, (h, w, 3))
        img[int(rng.integers(0, h))] = 255
    elif base == "white_col":
        img = rng.integers(0, 100, (h, w, 3))
        img[:, int(rng.integers(0, w))] = 255
    elif base == "white_margin":
        img = rng.integers(0, 200, (h, w, 3))
        img[:, w - w // 4:] = 255
        img[h - h // 8:] = 255
    elif base == "one_channel":
        img = np.full((h, w, 3), 255)
        img[..., 1] = rng.integers(0, 256, (h, w))
    elif base == "near_white_dark_px":
        img = rng.integers(251, 256, (h, w, 3))
        img[int(rng.integers(0, h)), int(rng.integers(0, w))] = (3, 2, 1)
    else:
        raise ValueError(kind)
    img = np.ascontiguousarray(img.astype(np.uint8))
    if kind.startswith("jpeg_"):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=95)
        img = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))
    return img


def reference_functions(utils_py: str):
    tree = ast.parse(open(utils_py).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("is_blank", "is_partly_blank")]
    assert len(keep) == 2, "the reference file does not define is_blank and is_partly_blank"
    ns = {"np": np, "Image": Image, "BytesIO": io.BytesIO}
    exec(compile(ast.Module(body=keep, type_ignores=[]), utils_py, "exec"), ns)
    return ns["is_blank"], ns["is_partly_blank"]


def main():
    is_blank, is_partly_blank = reference_functions(sys.argv[1])
    out = {"what": "image_status by the reference's is_blank / is_partly_blank on seeded images (see make_blank_golden.py)", "cases": []}
    for i, (kind, h, w) in enumerate(CASES):
        seed = 0xB1A2C000 + i
        img = build_image(kind, h, w, seed)
        im = Image.fromarray(img)
        st = "blank" if is_blank(im=im) else "partly blank" if is_partly_blank(im=im) else "complete"
        out["cases"].append({"kind": kind, "h": h, "w": w, "seed": seed, "sha256": hashlib.sha256(img.tobytes()).hexdigest(), "status": st})
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", len(out["cases"]), "cases:", sorted({c["status"] for c in out["cases"]}))


if __name__ == "__main__":
    main()
