"""The white-space key of a tile sweep (``detect.py --blank-key``): blank / partly blank / complete per image.

The reference makes a second pass over all of its JPEG tiles for this (reference src/utils.py:392-479, remove_white_image_boxes): it
decodes every tile again, calls ``is_blank`` (:325-349) and ``is_partly_blank`` (:352-369) on it and writes
``data/image_boxes_blank_key.csv`` with an ``image_status`` per tile.  Here the statistics those two functions need are taken from the
decoded tiles while they lie in HBM (csrc/blank_stats.hip, engine.blank_stats), nine integers per image:

    L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 per pixel    Pillow's convert("L"); l_min, l_max = getextrema()
    blank_rows   rows whose 3 w bytes sum to >= 750 w              np.average(im, axis=(1, 2)) >= 250.
    blank_cols   columns whose 3 h bytes sum to >= 750 h           np.average(im, axis=(0, 2)) >= 250.
    nonblank_px  pixels with max(R, G, B) < 250, and x0, y0, x1, y1 their bounding box (inclusive; none: w, h, -1, -1): the mask of
                 correct_partly_blank_geom (:507-510).  nonblank_px == 0 is the "partly blank" tile the reference later drops as "actually
                 blank" (:463-466).

(The integer forms equal the float ones: the sums are exact in float64, and (750 n - 1) / (3 n) is far from 250 for every n.)
``stats_numpy`` is the restatement of the kernel in numpy, for documentation and the CPU tests; ``status`` turns records into the
reference's three strings; the rest is the key file: per-rank part files appended batch by batch, merged at the end of the sweep into what
``DataFrame.to_csv`` gives the reference (an unnamed running index first), which its ``pd.read_csv(...)['image_status']`` reads unchanged.
"""
from __future__ import annotations

import glob
import os
import threading
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

FIELDS = ("l_min", "l_max", "blank_rows", "blank_cols", "nonblank_px", "x0", "y0", "x1", "y1")
BLANK, PARTLY_BLANK, COMPLETE = "blank", "partly blank", "complete"       # reference get_image_blank_status
NAME_COLUMNS = ("year", "bbox_ind", "x_offset", "y_offset")
COLUMNS = NAME_COLUMNS + ("image_status", "image") + FIELDS
HEADER = "," + ",".join(COLUMNS) + "\n"                                      # DataFrame.to_csv: the index column has no name
KEY_FILE = "image_boxes_blank_key.csv"


def stats_numpy(img: np.ndarray) -> np.ndarray:
    """One uint8 RGB image [h, w, 3] -> its nine statistics (int32 [9], FIELDS), in the integer arithmetic of the kernel."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.shape[0] > 0 and img.shape[1] > 0
    h, w = img.shape[:2]
    v = img.astype(np.int64)
    grey = (19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16
    rows = int((v.sum(axis=(1, 2)) >= 750 * w).sum())
    cols = int((v.sum(axis=(0, 2)) >= 750 * h).sum())
    mask = img.max(axis=2) < 250
    n = int(mask.sum())
    if n:
        ys, xs = np.nonzero(mask.any(axis=1))[0], np.nonzero(mask.any(axis=0))[0]
        box = (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))
    else:
        box = (w, h, -1, -1)
    return np.asarray((int(grey.min()), int(grey.max()), rows, cols, n) + box, np.int32)


def status(stats) -> List[str]:
    """Records int [n, 9] (or one [9]) -> the reference's image_status strings: is_blank, else is_partly_blank, else complete."""
    s = np.asarray(stats, dtype=np.int64).reshape(-1, len(FIELDS))
    lo, hi = s[:, 0], s[:, 1]
    blank = ((lo == 0) & (hi == 0)) | ((lo == 1) & (hi == 1)) | ((lo == 255) & (hi == 255)) | ((lo >= 250) & (hi >= 250))
    partly = s[:, 2] + s[:, 3] > 0
    return [BLANK if b else PARTLY_BLANK if p else COMPLETE for b, p in zip(blank.tolist(), partly.tolist())]


def name_fields(name: str) -> Tuple[str, str, str, str]:
    """(year, bbox_ind, x_offset, y_offset) of a tile name of the four-field form <prefix><year>_<bbox_ind>_<x_offset>_<y_offset>[.ext], as
    geocode.parse_stems reads it (reference generate_image_specs_from_file_name); four empty strings for any other name."""
    stem = os.path.basename(name)
    for ext in (".jpeg", ".jpg", ".tif", ".tiff", ".png"):
        if stem.lower().endswith(ext):
            stem = stem[:-len(ext)]
            break
    parts = stem.split("_")
    if len(parts) != 4 or len(parts[0]) < 4 or not parts[0][-4:].isdigit() or not all(p.isdigit() for p in parts[1:]):
        return "", "", "", ""
    return str(int(parts[0][-4:])), str(int(parts[1])), str(int(parts[2])), str(int(parts[3]))


def key_rows(names: Sequence[str], stats) -> List[str]:
    """One key line per image, without the index column and the newline: the COLUMNS from `year` on."""
    s = np.asarray(stats, dtype=np.int64).reshape(-1, len(FIELDS))
    assert s.shape[0] == len(names)
    rows = []
    for name, st, rec in zip(names, status(s), s.tolist()):
        image = os.path.basename(name)
        if any(c in image for c in ',"\r\n'):
            image = '"' + image.replace('"', '""') + '"'
        rows.append(",".join(name_fields(name) + (st, image) + tuple(str(v) for v in rec)))
    return rows


def part_path(directory: str, rank: int) -> str:
    return os.path.join(directory, f"blank_key.rank{rank}.csv")


class PartFile:
    """A rank's part of the key, ``blank_key.rank<r>.csv`` in the run directory: ``<order>,<key row>`` lines appended per batch (order = the
    image's place in the sweep's sorted source listing).  `append` returns when the lines are in the file (fsync'd when durable), so a tile
    the done-manifest records afterwards always has its row; a line a crash cut short is dropped when the file is opened again."""

    def __init__(self, directory: str, rank: int = 0):
        self.path = part_path(directory, rank)
        self._fd: Optional[int] = None
        self._lock = threading.Lock()                  # several writer threads append to one part

    def open(self) -> None:
        if os.path.exists(self.path):
            with open(self.path, "r+b") as r:
                data = r.read()
                r.truncate(data.rfind(b"\n") + 1)
        self._fd = os.open(self.path, os.O_WRONLY | os.O_CREAT | os.O_APPEND, 0o644)

    def append(self, order: Iterable[int], rows: Sequence[str], durable: bool = True) -> None:
        data = "".join(f"{int(o)},{r}\n" for o, r in zip(order, rows)).encode()
        if not data:
            return
        with self._lock:                               # one batch's lines stay together whichever writer thread gets here first
            view = memoryview(data)
            while view:
                view = view[os.write(self._fd, view):]
            if durable:
                os.fsync(self._fd)

    def close(self) -> None:
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None


def read_parts(directory: str) -> Dict[str, Tuple[int, str]]:
    """Every ``blank_key.rank*.csv`` of the directory (whatever the world size of the run that wrote it) -> {row: (order, row)} keyed by the
    row's image name; a last line without its newline is ignored, an image that appears twice keeps one row (the bytes are equal)."""
    found: Dict[str, Tuple[int, str]] = {}
    for path in sorted(glob.glob(os.path.join(directory, "blank_key.rank*.csv"))):
        with open(path, "rb") as f:
            data = f.read()
        end = data.rfind(b"\n")
        if end < 0:
            continue
        for line in data[:end].decode().split("\n"):
            if not line:
                continue
            order, row = line.split(",", 1)
            image = _image_of(row)
            if image not in found:
                found[image] = (int(order), row)
    return found


def _image_of(row: str) -> str:
    rest = row.split(",", 5)[5]                        # after year, bbox_ind, x_offset, y_offset, image_status
    if rest.startswith('"'):
        end = 1
        while True:
            end = rest.index('"', end)
            if rest[end:end + 2] != '""':
                return rest[:end + 1]
            end += 2
    return rest.split(",", 1)[0]


def merge_parts(directory: str, out_path: str, listing: Optional[Sequence[str]] = None) -> Dict[str, int]:
    """The key file from the directory's part files: rows in the order of the source listing (`listing`: the sweep's sorted file names, so
    that rows an interrupted run recorded under another listing fall into place; without it, or for a name it lacks, the recorded order,
    then the name), a running index in front, written to a temporary file and renamed.  Returns the number of rows per status."""
    place = {os.path.basename(n): i for i, n in enumerate(listing)} if listing is not None else {}
    rows = sorted(read_parts(directory).items(), key=lambda kv: (place.get(kv[0], len(place)), kv[1][0], kv[0]))
    counts = {BLANK: 0, PARTLY_BLANK: 0, COMPLETE: 0}
    tmp = out_path + ".tmp"
    with open(tmp, "w", newline="") as f:
        f.write(HEADER)
        for i, (_, (_, row)) in enumerate(rows):
            f.write(f"{i},{row}\n")
            counts[row.split(",", 5)[4]] += 1
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, out_path)
    return counts
