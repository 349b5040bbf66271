"""Water depth under every facility from a depth raster (``detect.py --bathymetry``, ``python -m aquaculture_amd.bathymetry``).

The reference's add_facility_depth (src/utils_tonnage.py:591-665, reached through AquaFacility.add_depth, :1066, and run by
src/Results/generate_facilities.py --bathymetry_statistic bathy_min): every facility's circle and square cages are united and carried to
EPSG:4326, ``rasterstats.zonal_stats(..., all_touched=True)`` takes min, max and mean of the EMODnet bathymetry cells the union touches,
and cage_depth is half the chosen statistic, floored at min_cage_threshold; a facility without a valid cell gets default_cage_depth.

The definition, which csrc/depth.hip (through engine.depth_stats) and stats_numpy both implement, byte for byte:

  cages      a facility's cages are its circle_farm and square_farm members (rectangles are left out, as in the reference), each the
             axis-parallel box lon_min, lon_max, lat_min, lat_max of geocode.py.  EPSG:3857 -> EPSG:4326 is separable, so the reference's
             re-projected boxes are these rectangles up to rounding.
  the grid   float32 [nrows, ncols], row 0 the northernmost, north-west corner (x0, y0), cell size dx, dy > 0: the window load_window
             cut out of the raster files.  Cell (r, c) is the half-open square [x0 + c dx, x0 + (c + 1) dx) x (y0 - (r + 1) dy, y0 - r dy].
  ranges     c0 = floor((lon_min - x0) / dx), c1 = floor((lon_max - x0) / dx), r0 = floor((y0 - lat_max) / dy), r1 = floor((y0 - lat_min) / dy)
             in fp64 (only - / floor, comparisons and selections), kept inside [-1, ncols] / [-1, nrows] in fp64 (what is not >= -1, a NaN
             included, gives -1) before the conversion to integers.  The cage touches columns c0 .. c1 and rows r0 .. r1, inclusive,
             intersected with the grid: a cell counts when the closed box meets the cell's half-open square, so an edge exactly on a cell
             boundary takes the cell to its east / south and not the one to its west / north.  A cage with a NaN coordinate touches nothing.
  touched    the union of the cages' cell rectangles; a cell several cages share counts once.  Valid cells: touched, not NaN, not equal
             to nodata.  count = their number; min and max = their float32 values widened (a zero is +0.0).
  sum        the facility's window is the bounding rectangle of its touched cells, flattened row-major to indices i.  Partial sum l
             (l = 0 .. 63) starts at +0.0 and adds the widened values of the valid cells with i % 64 == l in ascending i; the sum is the 64
             partials added in order of l, starting from +0.0.  mean = sum / count.
  columns    bathy_min = -min, bathy_max = -max, bathy_mean = bathy_depth = -mean (the raster is negative below sea level); all null
             with count == 0.  cage_depth = default_depth if the chosen statistic (bathy_min or bathy_depth) is null, else statistic / 2;
             then cage_depth = min_depth if cage_depth <= min_depth.

Raster files (no rasterio, GDAL or tifffile needed): ESRI ASCII grids (.asc, what EMODnet ships) and single-band GeoTIFFs through Pillow
(float32, float64 or int16; transform from the ModelPixelScale and ModelTiepoint tags, nodata from GDAL_NODATA).  Several files are
merged as ``rasterio.merge`` does by default: a cell's value comes from the first listed file that contains the cell, nodata or not.

NOT pinned, for want of GDAL / rasterio / rasterstats on the machines this was written on:
  * the tie rule.  GDAL's all-touched rasterisation is taken to assign a coordinate exactly on a cell boundary to the cell east / south of
    it (floor of the pixel coordinate); exact ties have measure zero for real coordinates.
  * the mean's last digits: rasterstats takes the mean in the raster's own dtype (float32 for EMODnet), here the float32 values are summed
    in fp64 in the order above.
  * the window's origin: cell indices are taken relative to the cropped window's corner x0 + C dx, y0 - R dy as rounded to fp64, GDAL's
    relative to the file's own corner; again a difference only within rounding of a cell boundary.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import facilities as aqfac
from . import geocode

STATISTICS = ("bathy_min", "bathy_depth")
DEPTH_COLUMNS = ("bathy_depth", "cage_depth", "bathy_min", "bathy_max", "bathy_mean")       # the reference's, in its order
DEPTHS_FILE = "facility_depths.csv"
DEFAULT_DEPTH, DEFAULT_MIN_DEPTH = 4.84, 1.0                # the reference README's values (tonnage.py's)
ORIGIN_TOLERANCE = 1e-6                                     # of a cell: how far files' origins may be from whole cells apart
_ASC_KEYS = ("ncols", "nrows", "xllcorner", "xllcenter", "yllcorner", "yllcenter", "cellsize", "dx", "dy", "nodata_value")
_ASC_CHUNK = 1 << 22                                        # numbers parsed per call


# ---- raster files ----

class Raster:
    """One raster file's geometry -- nrows, ncols, the north-west corner (x0, y0), the cell size (dx, dy), nodata (None: none) -- and
    read(r0, r1, c0, c1): the float32 cells of rows r0 .. r1 - 1 and columns c0 .. c1 - 1."""

    def __init__(self, path: str):
        self.path = path
        if path.lower().endswith((".tif", ".tiff")):
            self._tiff_header()
        else:
            self._asc_header()
        for name in ("x0", "y0", "dx", "dy"):
            if not math.isfinite(getattr(self, name)):
                raise ValueError(f"{path}: {name} = {getattr(self, name)} is not finite")
        if not (self.dx > 0 and self.dy > 0):
            raise ValueError(f"{path}: cell size {self.dx} x {self.dy}: only north-up rasters with positive cell sizes are read")
        if self.nrows < 1 or self.ncols < 1:
            raise ValueError(f"{path}: {self.nrows} rows of {self.ncols} cells")

    # ESRI ASCII grid: ncols nrows xllcorner|xllcenter yllcorner|yllcenter cellsize [dx dy] [NODATA_value], then the rows from the north

    def _asc_header(self) -> None:
        h: Dict[str, float] = {}
        with open(self.path, "rb") as f:
            while True:
                at = f.tell()
                tok = f.readline().split()
                if len(tok) == 2 and tok[0][:1].isalpha() and tok[0].decode("ascii", "replace").lower() in _ASC_KEYS:
                    try:
                        h[tok[0].decode().lower()] = float(tok[1])
                    except ValueError:
                        raise ValueError(f"{self.path}: header field {tok[0].decode()} = {tok[1]!r}") from None
                    continue
                self._body = at
                break
        try:
            self.ncols, self.nrows = int(h["ncols"]), int(h["nrows"])
            self.dx = h["dx"] if "dx" in h else h["cellsize"]
            self.dy = h["dy"] if "dy" in h else h["cellsize"]
            self.x0 = h["xllcorner"] if "xllcorner" in h else h["xllcenter"] - self.dx / 2
            south = h["yllcorner"] if "yllcorner" in h else h["yllcenter"] - self.dy / 2
        except KeyError as e:
            raise ValueError(f"{self.path}: not an ESRI ASCII grid: no {e.args[0]} in its header") from None
        self.y0 = south + self.nrows * self.dy
        self.nodata = h.get("nodata_value")

    def _asc_read(self, r0: int, r1: int, c0: int, c1: int) -> np.ndarray:
        """The text is parsed from its start down to row r1, `_ASC_CHUNK` numbers at a time, by numpy's C parsers: np.loadtxt (numpy >= 1.23)
        where every text line is one row of the grid, as EMODnet and GDAL write them, else np.fromfile, which takes any layout."""
        out = np.empty((r1 - r0, c1 - c0), np.float32)
        rows_per = max(1, _ASC_CHUNK // self.ncols)
        with open(self.path, "rb") as f:
            f.seek(self._body)
            r, by_line = 0, True
            while r < r1:
                n = min(rows_per, r1 - r)
                v = None
                if by_line:
                    at = f.tell()
                    try:
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")     # (an empty rest of the file warns; it is reported below)
                            v = np.loadtxt(f, dtype=np.float64, comments=None, max_rows=n, ndmin=2)
                    except ValueError:
                        v = None
                    if v is None or v.shape[1] != self.ncols:
                        by_line, v = False, None
                        f.seek(at)
                if v is None:
                    v = np.fromfile(f, dtype=np.float64, count=n * self.ncols, sep=" ")
                if v.size != n * self.ncols:
                    raise ValueError(f"{self.path}: the file ends in row {r + v.size // self.ncols} of {self.nrows}")
                if r + n > r0:
                    a = max(r, r0)
                    out[a - r0:r + n - r0] = v.reshape(n, self.ncols)[a - r:, c0:c1]
                r += n
        return out

    # GeoTIFF through Pillow

    def _tiff_open(self):
        from PIL import Image
        return Image.open(self.path)

    def _tiff_header(self) -> None:
        from PIL import Image
        limit = Image.MAX_IMAGE_PIXELS
        Image.MAX_IMAGE_PIXELS = None                       # a bathymetry mosaic is larger than what Pillow takes for a decompression bomb
        try:
            with self._tiff_open() as im:
                tags = dict(im.tag_v2)
                mode, (self.ncols, self.nrows) = im.mode, im.size
        finally:
            Image.MAX_IMAGE_PIXELS = limit
        spp = tags.get(277, 1)
        if int(spp[0] if isinstance(spp, tuple) else spp) != 1 or mode not in ("F", "I", "I;16", "I;16S", "I;16B"):
            raise ValueError(f"{self.path}: one band of float32, float64 or int16 is read, not {spp} samples per pixel in Pillow's mode {mode}")
        scale, tie, matrix = tags.get(33550), tags.get(33922), tags.get(34264)
        if matrix is not None:
            m = [float(v) for v in matrix]
            if len(m) != 16 or m[1] != 0.0 or m[4] != 0.0:
                raise ValueError(f"{self.path}: a rotated or sheared raster (ModelTransformation with off-diagonal terms): only north-up rasters are read")
            self.dx, self.dy, self.x0, self.y0 = m[0], -m[5], m[3], m[7]
        elif scale is not None and tie is not None and len(tie) >= 6 and len(scale) >= 2:
            self.dx, self.dy = float(scale[0]), float(scale[1])
            self.x0 = float(tie[3]) - float(tie[0]) * self.dx
            self.y0 = float(tie[4]) + float(tie[1]) * self.dy
        else:
            raise ValueError(f"{self.path}: no georeference: neither ModelPixelScale (33550) with ModelTiepoint (33922) nor ModelTransformation (34264)")
        nd = tags.get(42113)
        self.nodata = None
        if nd is not None:
            try:
                self.nodata = float(str(nd[0] if isinstance(nd, tuple) else nd).strip().strip("\x00"))
            except ValueError:
                raise ValueError(f"{self.path}: GDAL_NODATA = {nd!r}") from None

    def _tiff_read(self, r0: int, r1: int, c0: int, c1: int) -> np.ndarray:
        from PIL import Image
        limit = Image.MAX_IMAGE_PIXELS
        Image.MAX_IMAGE_PIXELS = None
        try:
            with self._tiff_open() as im:
                return np.asarray(im.crop((c0, r0, c1, r1))).astype(np.float32)
        finally:
            Image.MAX_IMAGE_PIXELS = limit

    def read(self, r0: int, r1: int, c0: int, c1: int) -> np.ndarray:
        if not (0 <= r0 <= r1 <= self.nrows and 0 <= c0 <= c1 <= self.ncols):
            raise ValueError(f"{self.path}: rows {r0} .. {r1}, columns {c0} .. {c1} of {self.nrows} x {self.ncols}")
        if r0 == r1 or c0 == c1:
            return np.zeros((r1 - r0, c1 - c0), np.float32)
        return (self._tiff_read if self.path.lower().endswith((".tif", ".tiff")) else self._asc_read)(r0, r1, c0, c1)


def load_window(paths: Sequence[str], bounds: Optional[Tuple[float, float, float, float]], pad: int = 1) -> dict:
    """The cells of the raster files that bound (lon_min, lon_max, lat_min, lat_max), one cell more on every side, clipped to the data ->
    {"data": float32 [nrows, ncols], "x0", "y0" (the window's north-west corner), "dx", "dy", "nodata" (None: none), "files", "offset":
    (row, column) of the window in the first file's grid}.  All files have the first one's cell size and origins whole cells from its
    own; a cell's value is that of the first listed file that contains the cell, nodata or not; a cell no file contains is NaN.  Files
    with another nodata value have it replaced by the first one's.  bounds = None (no cage), or bounds off the data: a window of no cells."""
    if isinstance(paths, str):
        paths = [paths]
    if not paths:
        raise ValueError("bathymetry: no raster file")
    files = [Raster(p) for p in paths]
    f0 = files[0]
    dx, dy = f0.dx, f0.dy
    place = []                                              # (file, its first row and column in the first file's grid)
    for f in files:
        if abs(f.dx - dx) > 1e-9 * dx or abs(f.dy - dy) > 1e-9 * dy:
            raise ValueError(f"{f.path}: cell size {f.dx} x {f.dy}, {f0.path} has {dx} x {dy}: the files of one call share the cell size")
        kx, ky = (f.x0 - f0.x0) / dx, (f0.y0 - f.y0) / dy
        if abs(kx - round(kx)) > ORIGIN_TOLERANCE or abs(ky - round(ky)) > ORIGIN_TOLERANCE:
            raise ValueError(f"{f.path}: its origin lies {kx} columns and {ky} rows from that of {f0.path}: not whole cells")
        place.append((f, int(round(ky)), int(round(kx))))
    nodata = next((f.nodata for f in files if f.nodata is not None), None)
    if nodata is not None:
        nodata = float(np.float32(nodata))                  # the value as the float32 cells can hold it
    out = {"x0": np.float64(f0.x0), "y0": np.float64(f0.y0), "dx": np.float64(dx), "dy": np.float64(dy), "nodata": nodata, "files": [f.path for f in files],
           "data": np.zeros((0, 0), np.float32), "offset": (0, 0)}
    if bounds is None or not all(math.isfinite(float(v)) for v in bounds):
        return out
    lon_min, lon_max, lat_min, lat_max = (np.float64(v) for v in bounds)
    big = float(1 << 40)
    cell = lambda t: int(min(max(math.floor(t), -big), big))
    C0, C1 = cell((lon_min - f0.x0) / dx) - pad, cell((lon_max - f0.x0) / dx) + pad + 1
    R0, R1 = cell((f0.y0 - lat_max) / dy) - pad, cell((f0.y0 - lat_min) / dy) + pad + 1
    C0, C1 = max(C0, min(c for _, _, c in place)), min(C1, max(c + f.ncols for f, _, c in place))
    R0, R1 = max(R0, min(r for _, r, _ in place)), min(R1, max(r + f.nrows for f, r, _ in place))
    if C0 >= C1 or R0 >= R1:
        return out
    data = np.full((R1 - R0, C1 - C0), np.nan, np.float32)
    for f, fr, fc in reversed(place):                       # the first listed file is written last: it wins
        a0, a1, b0, b1 = max(R0, fr), min(R1, fr + f.nrows), max(C0, fc), min(C1, fc + f.ncols)
        if a0 >= a1 or b0 >= b1:
            continue
        part = f.read(a0 - fr, a1 - fr, b0 - fc, b1 - fc)
        if f.nodata is not None and float(np.float32(f.nodata)) != nodata:
            part[part == np.float32(f.nodata)] = np.float32(nodata)
        data[a0 - R0:a1 - R0, b0 - C0:b1 - C0] = part
    out.update(data=data, x0=np.float64(f0.x0) + np.float64(C0) * np.float64(dx), y0=np.float64(f0.y0) - np.float64(R0) * np.float64(dy), offset=(R0, C0))
    return out


# ---- the cages ----

def cage_rows(table: Dict[str, np.ndarray]) -> np.ndarray:
    """bool per detection: a circle_farm or a square_farm."""
    cls = np.asarray(table["cls"], np.int64)
    return (cls == aqfac.CLS_OF["circle_farm"]) | (cls == aqfac.CLS_OF["square_farm"])


def table_bounds(table: Dict[str, np.ndarray], keep=None) -> Optional[Tuple[float, float, float, float]]:
    """(lon_min, lon_max, lat_min, lat_max) over the circle and square detections (with keep: those with keep[k]); None without any."""
    m = cage_rows(table)
    if keep is not None:
        m &= np.asarray(keep, bool)
    m &= np.isfinite(table["lon_min"]) & np.isfinite(table["lon_max"]) & np.isfinite(table["lat_min"]) & np.isfinite(table["lat_max"])
    if not m.any():
        return None
    return (float(np.min(table["lon_min"][m])), float(np.max(table["lon_max"][m])), float(np.min(table["lat_min"][m])), float(np.max(table["lat_max"][m])))


def facility_cages(fac: Dict[str, list], table: Dict[str, np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """(entry_start int32 [F + 1], cages float64 [E, 4]: lon_min, lon_max, lat_min, lat_max) of facilities.cluster's result: facility f owns
    the entries entry_start[f] .. entry_start[f + 1] - 1, its circle and square members in ascending cage id."""
    is_cage = cage_rows(table)
    start, ids = [0], []
    for members in fac["cage_ids"]:
        ids.extend(c for c in sorted(int(c) for c in members) if is_cage[c])
        start.append(len(ids))
    ids_a = np.asarray(ids, np.int64)
    cages = np.stack([np.asarray(table[c], np.float64)[ids_a] for c in ("lon_min", "lon_max", "lat_min", "lat_max")], 1).reshape(-1, 4)
    return np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(cages)


# ---- the restatement ----

def _check_entries(entry_start, cages) -> Tuple[np.ndarray, np.ndarray]:
    entry_start = np.ascontiguousarray(entry_start, dtype=np.int32).reshape(-1)
    cages = np.ascontiguousarray(cages, dtype=np.float64).reshape(-1, 4)
    if entry_start.shape[0] < 1 or entry_start[0] < 0 or entry_start[-1] > cages.shape[0] or (np.diff(entry_start) < 0).any():
        raise ValueError("bathymetry: entry offsets have to be non-decreasing inside the cages")
    return entry_start, cages


def cell_ranges_numpy(entry_start, cages, nrows: int, ncols: int, x0, y0, dx, dy) -> Tuple[np.ndarray, np.ndarray]:
    """(cage ranges int32 [E, 4], facility windows int32 [F, 4]), each (c0, c1, r0, r1) inclusive and (0, -1, 0, -1) when empty."""
    entry_start, cages = _check_entries(entry_start, cages)
    x0, y0, dx, dy = np.float64(x0), np.float64(y0), np.float64(dx), np.float64(dy)
    F = entry_start.shape[0] - 1

    def cell(t, n):
        f = np.floor(t)
        return np.where(f >= -1.0, np.where(f > float(n), float(n), f), -1.0).astype(np.int64)

    with np.errstate(all="ignore"):
        c0, c1 = cell((cages[:, 0] - x0) / dx, ncols), cell((cages[:, 1] - x0) / dx, ncols)
        r0, r1 = cell((y0 - cages[:, 3]) / dy, nrows), cell((y0 - cages[:, 2]) / dy, nrows)
    c0, c1, r0, r1 = np.maximum(c0, 0), np.minimum(c1, ncols - 1), np.maximum(r0, 0), np.minimum(r1, nrows - 1)
    some = (c0 <= c1) & (r0 <= r1) & ~np.isnan(cages).any(1)
    empty = np.array([0, -1, 0, -1], np.int64)
    ranges = np.where(some[:, None], np.stack([c0, c1, r0, r1], 1), empty[None, :]).reshape(-1, 4)
    owner = np.repeat(np.arange(F), np.diff(entry_start))
    first = int(entry_start[0])
    of = owner[some[first:first + owner.shape[0]]]
    rs = ranges[first:first + owner.shape[0]][some[first:first + owner.shape[0]]]
    big = np.iinfo(np.int64).max
    lo_c, hi_c, lo_r, hi_r = np.full(F, big), np.full(F, -1), np.full(F, big), np.full(F, -1)
    np.minimum.at(lo_c, of, rs[:, 0]); np.maximum.at(hi_c, of, rs[:, 1]); np.minimum.at(lo_r, of, rs[:, 2]); np.maximum.at(hi_r, of, rs[:, 3])
    has = hi_c >= 0
    windows = np.where(has[:, None], np.stack([lo_c, hi_c, lo_r, hi_r], 1), empty[None, :]).reshape(-1, 4)
    return ranges.astype(np.int32), windows.astype(np.int32)


def stats_numpy(entry_start, cages, grid: dict) -> Tuple[np.ndarray, np.ndarray]:
    """(stats float64 [F, 3]: min, max, sum; count int64 [F]) by the module docstring's definition, as csrc/depth.hip computes them."""
    entry_start, cages = _check_entries(entry_start, cages)
    data = np.asarray(grid["data"], np.float32)
    nodata = grid.get("nodata")
    ranges, windows = cell_ranges_numpy(entry_start, cages, data.shape[0], data.shape[1], grid["x0"], grid["y0"], grid["dx"], grid["dy"])
    F = windows.shape[0]
    stats = np.empty((F, 3), np.float64)
    stats[:] = (np.inf, -np.inf, 0.0)
    count = np.zeros(F, np.int64)
    for f in range(F):
        c0, c1, r0, r1 = (int(v) for v in windows[f])
        if c1 < c0:
            continue
        touched = np.zeros((r1 - r0 + 1, c1 - c0 + 1), bool)
        for a0, a1, b0, b1 in ranges[entry_start[f]:entry_start[f + 1]].tolist():
            if a1 >= a0:
                touched[b0 - r0:b1 - r0 + 1, a0 - c0:a1 - c0 + 1] = True
        v = data[r0:r1 + 1, c0:c1 + 1].astype(np.float64)
        valid = touched & ~np.isnan(v)
        if nodata is not None:
            valid &= v != np.float64(nodata)
        n = int(valid.sum())
        if n == 0:
            continue
        flat = np.where(valid, v, 0.0).reshape(-1)          # (adding +0.0 changes no partial: each starts at +0.0)
        rows = -(-flat.shape[0] // 64)
        m = np.zeros((rows + 1, 64))                        # row 0: where the partials start
        m.reshape(-1)[64:64 + flat.shape[0]] = flat
        with np.errstate(all="ignore"):
            partial = np.add.accumulate(m, axis=0)[-1]
            total = np.add.accumulate(np.concatenate([[0.0], partial]))[-1]
        stats[f] = (v[valid].min() + 0.0, v[valid].max() + 0.0, total)
        count[f] = n
    return stats, count


def stats_gpu(entry_start, cages, grid: dict, times: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """stats_numpy's result from the GPU (engine.depth_stats: only the window is uploaded).  Raises without the library or a GPU."""
    import torch
    from . import engine
    entry_start, cages = _check_entries(entry_start, cages)
    data = np.ascontiguousarray(grid["data"], dtype=np.float32)
    stats, count, _ = engine.depth_stats(torch.from_numpy(entry_start).cuda(), torch.from_numpy(cages).cuda(), torch.from_numpy(data).cuda(),
                                         float(grid["x0"]), float(grid["y0"]), float(grid["dx"]), float(grid["dy"]), grid.get("nodata"), times=times)
    return stats.cpu().numpy(), count.cpu().numpy()


# ---- the columns ----

def depth_columns(stats, count, statistic: str = "bathy_min", default_depth: float = DEFAULT_DEPTH, min_depth: float = DEFAULT_MIN_DEPTH) -> Dict[str, list]:
    """The reference's five columns (None = null) and ``cells``, the number of valid cells, from min / max / sum and count."""
    if statistic not in STATISTICS:
        raise ValueError(f"bathymetry: the statistic is one of {', '.join(STATISTICS)}, not {statistic!r}")
    out: Dict[str, list] = {c: [] for c in (*DEPTH_COLUMNS, "cells")}
    num = lambda v: v if math.isfinite(v) else None
    for (mn, mx, sm), n in zip(np.asarray(stats, np.float64).reshape(-1, 3).tolist(), np.asarray(count, np.int64).tolist()):
        row = {"bathy_min": None, "bathy_max": None, "bathy_mean": None}
        if n > 0:
            row = {"bathy_min": num(-mn), "bathy_max": num(-mx), "bathy_mean": num(-(sm / float(n)))}
        row["bathy_depth"] = row["bathy_mean"]
        depth = float(default_depth) if row[statistic] is None else row[statistic] / 2
        if depth <= min_depth:
            depth = float(min_depth)
        row["cage_depth"] = depth
        for c in DEPTH_COLUMNS:
            out[c].append(row[c])
        out["cells"].append(int(n))
    return out


def facility_depths(fac: Dict[str, list], table: Dict[str, np.ndarray], grid: dict, statistic: str = "bathy_min",
                    default_depth: float = DEFAULT_DEPTH, min_depth: float = DEFAULT_MIN_DEPTH, cpu: bool = False, times: Optional[dict] = None) -> Dict[str, list]:
    """depth_columns of facilities.cluster's facilities over `grid` (load_window's).  cpu: stats_numpy instead of the GPU -- the same bytes."""
    entry_start, cages = facility_cages(fac, table)
    stats, count = stats_numpy(entry_start, cages, grid) if cpu else stats_gpu(entry_start, cages, grid, times)
    return depth_columns(stats, count, statistic, default_depth, min_depth)


def settings(paths: Sequence[str], table: Dict[str, np.ndarray], keep=None, statistic: str = "bathy_min", default_depth: float = DEFAULT_DEPTH,
             min_depth: float = DEFAULT_MIN_DEPTH) -> dict:
    """What facilities.facilities_from_table and tonnage.tonnage_from_table take as ``bathymetry``: the window of the files under the
    table's cages (read once for both) and the depth rule's three settings."""
    if statistic not in STATISTICS:
        raise ValueError(f"bathymetry: the statistic is one of {', '.join(STATISTICS)}, not {statistic!r}")
    return {"grid": load_window(paths, table_bounds(table, keep)), "statistic": statistic, "default_depth": float(default_depth), "min_depth": float(min_depth)}


def depths_of(fac: Dict[str, list], table: Dict[str, np.ndarray], bathymetry: dict, cpu: bool = False) -> Dict[str, list]:
    return facility_depths(fac, table, bathymetry["grid"], bathymetry["statistic"], bathymetry["default_depth"], bathymetry["min_depth"], cpu)


def describe_settings(bathymetry: dict) -> dict:
    """The record tonnage.json keeps: the raster names, the statistic."""
    return {"files": [os.path.basename(p) for p in bathymetry["grid"]["files"]], "statistic": bathymetry["statistic"]}


# ---- files ----

def write_depths_csv(path: str, fac: Dict[str, list], cols: Dict[str, list], by: str = "pass") -> int:
    """facility_index, `by`, cage_depth, bathy_depth, bathy_min, bathy_max, bathy_mean, cells: floats by ``repr``, nulls empty.
    tonnage.read_depths (--tonnage-depths) takes the file as it stands.  Returns the number of facilities that fell back to the default
    depth for want of a valid cell."""
    txt = lambda v: "" if v is None else repr(float(v))
    with open(path, "w") as f:
        f.write(f"facility_index,{by},cage_depth,bathy_depth,bathy_min,bathy_max,bathy_mean,cells\n")
        for k, fi in enumerate(fac["facility_index"]):
            f.write(",".join([str(int(fi)), str(fac[by][k]), *(txt(cols[c][k]) for c in ("cage_depth", "bathy_depth", "bathy_min", "bathy_max", "bathy_mean")),
                              str(cols["cells"][k])]) + "\n")
    return sum(1 for n in cols["cells"] if n == 0)


def add_options(p: argparse.ArgumentParser) -> None:
    """The options detect.py and this module's command line share."""
    p.add_argument("--bathymetry", nargs="+", default=None, metavar="FILE",
                   help="depth rasters (ESRI ASCII grids as EMODnet ships them, or single-band GeoTIFFs; of several files the first listed one "
                        "that contains a cell gives its value): every facility's cage depth becomes half the water depth under its circle and "
                        "square cages (the reference's add_facility_depth, src/utils_tonnage.py:591-665), the cells taken on the GPU")
    p.add_argument("--bathymetry-statistic", choices=STATISTICS, default="bathy_min",
                   help="the water depth of a facility: bathy_min, the deepest cell its cages touch, or bathy_depth, the mean over them")


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.bathymetry",
                                description="Cage depths of the facilities of an existing label directory from depth rasters, without running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv")
    p.add_argument("--out", default=None, metavar="CSV", help=f"default <labels>/../{DEPTHS_FILE}")
    p.add_argument("--land", default=None, metavar="GEOJSON", help="land polygons: only the detections at sea take part (the --land-filter step)")
    p.add_argument("--image-size", nargs=2, type=int, default=[geocode.IM_WIDTH, geocode.IM_HEIGHT], metavar=("W", "H"),
                   help="pixel size of the images (the border test of the circle areas)")
    p.add_argument("--tonnage-default-depth", type=float, default=DEFAULT_DEPTH, metavar="M", help="cage depth of a facility without a valid cell")
    p.add_argument("--tonnage-min-depth", type=float, default=DEFAULT_MIN_DEPTH, metavar="M", help="smallest cage depth (reference min_cage_threshold)")
    p.add_argument("--cpu", action="store_true", help="the numpy restatement instead of the GPU (the same bytes)")
    aqfac.add_options(p)
    p.set_defaults(facilities_by="pass")                    # the facilities --tonnage makes: --tonnage-depths takes the file
    add_options(p)
    opt = p.parse_args(argv)
    if not opt.bathymetry:
        p.error("--bathymetry FILE [FILE ...] is needed")
    out = opt.out or os.path.join(os.path.dirname(os.path.abspath(opt.labels.rstrip("/"))), DEPTHS_FILE)
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    keep = None
    if opt.land:
        from . import land as aqland
        keep = aqland.ocean_rows(table, aqland.load_land_geojson(opt.land), cpu=opt.cpu)
    fac = aqfac.cluster(table, opt.facilities_by, opt.facilities_conf, opt.facilities_eps, opt.facilities_min_cages, opt.image_size[0], opt.image_size[1],
                        labels_fn=aqfac.dbscan_numpy if opt.cpu else None, keep=keep)
    bathy = settings(opt.bathymetry, table, keep, opt.bathymetry_statistic, opt.tonnage_default_depth, opt.tonnage_min_depth)
    cols = depths_of(fac, table, bathy, cpu=opt.cpu)
    missing = write_depths_csv(out, fac, cols, opt.facilities_by)
    shape = bathy["grid"]["data"].shape
    print(f"{len(fac['facility_index'])} facilities, {missing} without a valid cell (default depth), window {shape[0]} x {shape[1]} cells, in {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
