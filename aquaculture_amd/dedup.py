"""One year's cages per tile and image pass (``detect.py --dedup-years``, ``python -m aquaculture_amd.dedup``).

The reference's dedup_cages_in_overlap_years_with_white_space (src/utils_tonnage.py:668-911), which AquaFacility.deduplicate_and_cluster
(:979-995) runs before every clustering by pass: an image pass spans three to five years, the same tile (bbox_ind, x_offset, y_offset) is
usually photographed in several of them, and without this step the same physical cage counts once per year.  Per pass and tile key the
reference puts the images that are not blank in some order; the first keeps its whole non-blank polygon, every later one its polygon minus
everything before it (tile_coverage), and a cage survives iff its box intersects the region allotted to its own image
(filter_cages_to_image_boxes; touching counts).  The order is a random shuffle, or the permutation with the smallest / largest summed
``area`` of the tile's surviving cages (img_box_allocation_in_tile).

All images of one tile key share one pixel grid and --blank-geom writes the exact pixel ring of the polygon (``ring_px``), so the step is
exact in integers.  The definitions (include/aq_engine.h):

    mask      complete image: the whole frame.  Partly blank image with a feature in the blank-geom file: pixel (c, r) is in the mask iff an
              odd number of vertical unit edges of the ring in row r lie at x <= c -- the even-odd fill of the exterior ring: pixels, holes
              and islands, the region of the reference's Polygon(exterior).  Blank images and partly blank images without a feature
              ("actually blank") take no part; their cages are dropped under every selection, as the reference's left merge drops them.
    window    the closed pixel box [xmin, xmax] x [ymin, ymax] of the geocoded table meets the closed pixel square (c, r) iff
              xmin - 1 <= c <= xmax and ymin - 1 <= r <= ymax: that range, clipped to the frame.  Empty: the cage survives nowhere.
    word      for a cage of slot i in a group of n <= 5 images (slots in ascending year): bit S of a uint32 is set iff some pixel of the
              window lies in exactly the masks of the slot set S, and i is in S.
    survival  under a permutation: some set S of the word has i before every other member of S.  This equals "the window meets mask_i minus
              the union of the earlier masks" and needs the pixels once for all n! orders; selections_literal is that literal form.
    min, max  permutations in itertools.permutations(range(n)) order; the area of one = the ``area`` of its surviving cages added one at a
              time in ascending row number from +0.0, NaN as 0.  max: the last whose area is >= the running best (from 0); min: the first
              whose area is < the running best (from +inf): the reference's comparisons at :770-775.
    random    the slots in ascending (u_j, j), u_j = tonnage.uniform(seed, bbox_ind, x_offset, y_offset, year_j): the project's Philox
              counters, so the order depends only on the seed and the image (the reference's sample(frac=1) is unseeded).

Three kernels (csrc/dedup.hip through engine.dedup_fill / dedup_sets / dedup_select) compute bitmaps, words and selections;
fill_numpy / sets_numpy / select_numpy restate them step by step and give the same bytes (``--cpu``).  Every cage gets the bits
SEL_MIN | SEL_MAX | SEL_RANDOM (tonnage.py's values) of the selections it survives.
"""
from __future__ import annotations

import argparse
import csv
import itertools
import json
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import blank as aqblank
from . import facilities as aqfac
from . import geocode
from .tonnage import SEL_MAX, SEL_MIN, SEL_RANDOM, uniform

FRAME = 1024                                                # the frame the geocoding and blank_geom.to_bounds assume
MAX_SLOTS, MAX_PERMS = 5, 120                               # the longest pass of facilities.IMAGE_PASSES; 5!
MAX_SIDE = 1 << 15
KIND_ABSENT, KIND_FULL, KIND_BITMAP = 0, 1, 2
BUDGET_BYTES = 256 << 20                                    # of bitmaps per call
SELECTIONS = {"random": SEL_RANDOM, "min": SEL_MIN, "max": SEL_MAX}
CAGES_FILE, TILES_FILE, JSON_FILE = "dedup_cages.csv", "dedup_tiles.csv", "dedup.json"
_FACT = (1, 1, 2, 6, 24, 120)


def pitch_words(w: int) -> int:
    """Words of a bitmap row: w pixels and the column x = w of the toggles."""
    return (int(w) + 32) // 32


# ---- the problem: groups of slots, cages ----

def make_problem(w, h, slots: Sequence[Sequence[Optional[Sequence[Tuple[int, int]]]]], cage_group, cage_slot, box, area, random_order=None,
                 names: Optional[Sequence[str]] = None) -> dict:
    """Group g has the frame w[g] x h[g] and the slots slots[g]: None for a complete image (the whole frame), else the closed pixel ring
    [(x, y), ...] (first vertex repeated at the end, axis-parallel, inside [0, w] x [0, h]).  Cage e belongs to slot cage_slot[e] of group
    cage_group[e] (-1: its image takes no part) and has the pixel box box[e] = (xmin, xmax, ymin, ymax) and the area area[e]; the cages
    are in ascending row number.  random_order [G, 5]: the slots of the random selection in order, padded with -1 (default: 0, 1, ..).
    names[g]: how a refusal calls the group.  Refused: a group of more than five images, a ring that leaves the frame or is not closed
    and axis-parallel, a cage that names a group or slot that does not exist."""
    w, h = np.asarray(w, np.int64).reshape(-1), np.asarray(h, np.int64).reshape(-1)
    G = w.shape[0]
    names = [f"group {g}" for g in range(G)] if names is None else list(names)
    if h.shape[0] != G or len(slots) != G or len(names) != G:
        raise ValueError("dedup: w, h, slots and names have to have one entry per group")
    slots = [list(s) for s in slots]
    for g in range(G):
        if not 1 <= len(slots[g]) <= MAX_SLOTS:
            raise ValueError(f"dedup: {names[g]} has {len(slots[g])} images; a group takes 1 to {MAX_SLOTS} (the longest image pass has {MAX_SLOTS} years)")
        if not (1 <= w[g] <= MAX_SIDE and 1 <= h[g] <= MAX_SIDE):
            raise ValueError(f"dedup: {names[g]} has a frame of {w[g]} x {h[g]} pixels (1 to {MAX_SIDE} a side)")
        for j, ring in enumerate(slots[g]):
            if ring is None:
                continue
            r = np.asarray(ring, np.int64).reshape(-1, 2)
            slots[g][j] = r
            if r.shape[0] < 4 or (r[0] != r[-1]).any():
                raise ValueError(f"dedup: the ring of image {j} of {names[g]} is not a closed walk")
            if (r < 0).any() or (r[:, 0] > w[g]).any() or (r[:, 1] > h[g]).any():
                raise ValueError(f"dedup: the ring of image {j} of {names[g]} has a vertex outside the {w[g]} x {h[g]} frame")
            d = np.diff(r, axis=0)
            if ((d[:, 0] != 0) & (d[:, 1] != 0)).any():
                raise ValueError(f"dedup: the ring of image {j} of {names[g]} has a segment that is not axis-parallel")
    cage_group, cage_slot = np.asarray(cage_group, np.int64).reshape(-1), np.asarray(cage_slot, np.int64).reshape(-1)
    box = np.asarray(box, np.int64).reshape(-1, 4)
    area = np.asarray(area, np.float64).reshape(-1)
    C = cage_group.shape[0]
    if cage_slot.shape[0] != C or box.shape[0] != C or area.shape[0] != C:
        raise ValueError("dedup: cage_group, cage_slot, box and area have to have one entry per cage")
    n_of = np.asarray([len(s) for s in slots], np.int64)
    if C and ((cage_group < -1).any() or (cage_group >= G).any() or (cage_slot < -1).any() or
              (cage_slot[cage_group >= 0] >= n_of[cage_group[cage_group >= 0]]).any()):
        raise ValueError("dedup: a cage names a group or a slot that does not exist")
    if random_order is None:
        random_order = [[j if j < len(s) else -1 for j in range(MAX_SLOTS)] for s in slots]
    random_order = np.asarray(random_order, np.int32).reshape(-1, MAX_SLOTS)
    for g in range(G):
        if sorted(random_order[g, :n_of[g]].tolist()) != list(range(n_of[g])):
            raise ValueError(f"dedup: the random order of {names[g]} is not a permutation of its {n_of[g]} images")
    return {"w": w, "h": h, "slots": slots, "n": n_of, "cage_group": cage_group, "cage_slot": cage_slot, "box": np.clip(box, -(1 << 30), 1 << 30),
            "area": area, "random_order": np.ascontiguousarray(random_order), "names": names}


def group_words(p: dict) -> np.ndarray:
    """int64 [G]: the bitmap words of every group (its rings' h rows x pitch_words(w))."""
    return np.asarray([sum(r is not None for r in s) * int(h) * pitch_words(w) for s, w, h in zip(p["slots"], p["w"], p["h"])], np.int64)


def chunks(p: dict, budget: int = BUDGET_BYTES) -> List[Tuple[int, int]]:
    """Consecutive group ranges whose bitmaps stay under `budget` bytes (a single group may exceed it) and 2^31 words."""
    words = group_words(p)
    limit = max(1, min(int(budget) // 4, (1 << 31) - 1))
    out, g0, acc = [], 0, 0
    for g in range(words.shape[0]):
        if g > g0 and acc + words[g] > limit:
            out.append((g0, g))
            g0, acc = g, 0
        acc += int(words[g])
    if words.shape[0] > g0:
        out.append((g0, words.shape[0]))
    return out


def tables(p: dict, g0: int = 0, g1: Optional[int] = None) -> Dict[str, np.ndarray]:
    """The arrays the three launchers take, for the groups g0 .. g1 - 1 and their cages (those whose image takes no part in any group are
    left out: they survive nothing).  ``rows``: the cages' indices in the problem, ascending inside every group."""
    g1 = len(p["slots"]) if g1 is None else g1
    G = g1 - g0
    group = np.zeros((G, 16), np.int32)
    xy, start, frame = [], [0], []
    word = 0
    for g in range(g0, g1):
        w, h = int(p["w"][g]), int(p["h"][g])
        group[g - g0, :3] = (len(p["slots"][g]), w, h)
        for j, ring in enumerate(p["slots"][g]):
            if ring is None:
                group[g - g0, 4 + j] = KIND_FULL
                continue
            group[g - g0, 4 + j], group[g - g0, 9 + j] = KIND_BITMAP, word
            xy.append(ring)
            start.append(start[-1] + ring.shape[0])
            frame.append((word, w, h, 0))
            word += h * pitch_words(w)
    if word >= 1 << 31:
        raise ValueError(f"dedup: bitmaps of {word} words for groups {g0} .. {g1 - 1} (fewer than 2^31 in one call): pass fewer groups at a time")
    cg = p["cage_group"]
    rows = np.nonzero((cg >= g0) & (cg < g1))[0]
    rows = rows[np.argsort(cg[rows], kind="stable")]
    cage = np.zeros((rows.shape[0], 8), np.int32)
    cage[:, 0], cage[:, 1], cage[:, 2:6] = cg[rows] - g0, p["cage_slot"][rows], p["box"][rows]
    return {"ring_xy": np.ascontiguousarray(np.concatenate(xy, 0) if xy else np.zeros((0, 2)), dtype=np.int32),
            "ring_start": np.asarray(start, np.int32), "ring_frame": np.asarray(frame, np.int32).reshape(-1, 4), "bitmap_words": word,
            "group": group, "cage": cage, "cage_start": np.searchsorted(cg[rows] - g0, np.arange(G + 1)).astype(np.int32),
            "area": np.ascontiguousarray(p["area"][rows]), "random_order": np.ascontiguousarray(p["random_order"][g0:g1]), "rows": rows}


# ---- the restatement of the three kernels ----

def fill_numpy(ring_xy, ring_start, ring_frame, bitmap_words: int) -> np.ndarray:
    """aq_dedup_fill_u32: the toggles of every vertical ring segment, then the inclusive prefix XOR of every row (shift-XOR inside a word,
    the parity carried across words) -> bitmap uint32 [bitmap_words]."""
    ring_xy = np.asarray(ring_xy, np.int64).reshape(-1, 2)
    ring_start, ring_frame = np.asarray(ring_start, np.int64), np.asarray(ring_frame, np.int64).reshape(-1, 4)
    bitmap = np.zeros(int(bitmap_words), np.uint32)
    for r in range(ring_frame.shape[0]):
        word0, w, h, _ = ring_frame[r].tolist()
        pitch = pitch_words(w)
        v = ring_xy[ring_start[r]:ring_start[r + 1]]
        a, b = v[:-1], v[1:]
        up = (a[:, 0] == b[:, 0]) & (a[:, 0] >= 0) & (a[:, 0] <= w)
        x = a[up, 0]
        y0, y1 = np.clip(np.minimum(a[up, 1], b[up, 1]), 0, h), np.clip(np.maximum(a[up, 1], b[up, 1]), 0, h)
        cnt = y1 - y0
        xs = np.repeat(x, cnt)
        ys = np.repeat(y0, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        np.bitwise_xor.at(bitmap, word0 + ys * pitch + (xs >> 5), (np.uint32(1) << (xs & 31).astype(np.uint32)).astype(np.uint32))
        rows = bitmap[word0:word0 + h * pitch].reshape(h, pitch)               # a view
        carry = np.zeros(h, np.uint32)
        for k in range(pitch):
            t = rows[:, k].copy()
            for s in (1, 2, 4, 8, 16):
                t ^= t << np.uint32(s)
            t ^= carry
            carry = np.where(t >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0)).astype(np.uint32)
            rows[:, k] = t
    return bitmap


def sets_numpy(group, cage, bitmap) -> np.ndarray:
    """aq_dedup_sets_u32: the cages' set words, uint32 [C], from the (row, word column) positions of every window."""
    group, cage = np.asarray(group, np.int64).reshape(-1, 16), np.asarray(cage, np.int64).reshape(-1, 8)
    bitmap = np.asarray(bitmap).view(np.uint32)
    ones = np.uint32(0xFFFFFFFF)
    out = np.zeros(cage.shape[0], np.uint32)
    for e in range(cage.shape[0]):
        g, i, xmin, xmax, ymin, ymax = cage[e, :6].tolist()
        if not 0 <= g < group.shape[0]:
            continue
        n, w, h = group[g, :3].tolist()
        n = min(max(n, 0), MAX_SLOTS)
        if not 0 <= i < n or group[g, 4 + i] not in (KIND_FULL, KIND_BITMAP):
            continue
        x0, x1, y0, y1 = max(xmin - 1, 0), min(xmax, w - 1), max(ymin - 1, 0), min(ymax, h - 1)
        if x0 > x1 or y0 > y1:
            continue
        pitch, k0, k1 = pitch_words(w), x0 >> 5, x1 >> 5
        cols = np.full(k1 - k0 + 1, ones, np.uint32)
        cols[0] &= ones << np.uint32(x0 & 31)
        cols[-1] &= ones >> np.uint32(31 - (x1 & 31))
        m = []
        for j in range(n):
            kind, off = int(group[g, 4 + j]), int(group[g, 9 + j])
            if kind == KIND_FULL:
                m.append(np.broadcast_to(ones, (y1 - y0 + 1, k1 - k0 + 1)))
            elif kind == KIND_BITMAP and 0 <= off and off + h * pitch <= bitmap.shape[0]:
                m.append(bitmap[off:off + h * pitch].reshape(h, pitch)[y0:y1 + 1, k0:k1 + 1])
            else:
                m.append(np.zeros((y1 - y0 + 1, k1 - k0 + 1), np.uint32))
        base = m[i] & cols[None, :]
        if not base.any():
            continue
        word = 0
        for S in range(1 << n):
            if not (S >> i) & 1:
                continue
            t = base
            for j in range(n):
                if j != i:
                    t = t & (m[j] if (S >> j) & 1 else ~m[j])
            if t.any():
                word |= 1 << S
        out[e] = word
    return out


def order_masks(order: Sequence[int], n: int) -> List[int]:
    """For every slot i < 5: the slot sets (as bits of a word) that hold no slot placed before i under `order` (the slots in order; one that
    is not named comes last); 0 for i >= n."""
    pos = [n] * MAX_SLOTS
    for k in range(min(n, len(order)) - 1, -1, -1):
        if 0 <= order[k] < n:
            pos[order[k]] = k
    out = []
    for i in range(MAX_SLOTS):
        before = sum(1 << j for j in range(n) if pos[j] < pos[i])
        out.append(sum(1 << S for S in range(32) if not S & before) if i < n else 0)
    return out


_PERMS = {n: list(itertools.permutations(range(n))) for n in range(1, MAX_SLOTS + 1)}
_PERM_MASKS = {n: np.asarray([order_masks(q, n) for q in _PERMS[n]], np.uint32) for n in _PERMS}


def select_numpy(group, cage_start, cage, words, area, random_order) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """aq_dedup_select_f64 -> (sel uint8 [C], chosen int32 [G, 4], sums float64 [G, 120]): per group the n! area sums, each cage added in
    turn to all of them; one ordered walk for min and max; the selections' bits."""
    group, cage = np.asarray(group, np.int64).reshape(-1, 16), np.asarray(cage, np.int64).reshape(-1, 8)
    words, area = np.asarray(words).view(np.uint32), np.asarray(area, np.float64)
    cage_start, random_order = np.asarray(cage_start, np.int64), np.asarray(random_order, np.int64).reshape(-1, MAX_SLOTS)
    G, C = group.shape[0], cage.shape[0]
    sel, chosen, sums = np.zeros(C, np.uint8), np.zeros((G, 4), np.int32), np.zeros((G, MAX_PERMS), np.float64)
    for g in range(G):
        n = min(max(int(group[g, 0]), 1), MAX_SLOTS)
        first = min(max(int(cage_start[g]), 0), C)
        end = min(max(int(cage_start[g + 1]), first), C)
        M = _PERM_MASKS[n]
        s = np.zeros(_FACT[n], np.float64)
        for e in range(first, end):
            i = int(cage[e, 1])
            if 0 <= i < n:
                a = area[e]
                s = np.where((words[e] & M[:, i]) != 0, s + (0.0 if a != a else a), s)
        sums[g, :_FACT[n]] = s
        best_max, best_min, qmax, qmin = 0.0, np.inf, -1, -1
        for q, v in enumerate(s.tolist()):
            if v >= best_max:
                qmax, best_max = q, v
            if v < best_min:
                qmin, best_min = q, v
        order = [int(j) for j in random_order[g]]
        Mr = order_masks(order, n)
        named = [j for j in order[:n] if 0 <= j < n]
        full = tuple(dict.fromkeys(named + [j for j in range(n) if j not in named]))
        chosen[g] = (qmin, qmax, _PERMS[n].index(full), _FACT[n])
        Mn = M[qmin].tolist() if qmin >= 0 else [0] * MAX_SLOTS
        Mx = M[qmax].tolist() if qmax >= 0 else [0] * MAX_SLOTS
        for e in range(first, end):
            i, wd = int(cage[e, 1]), int(words[e])
            if 0 <= i < n:
                sel[e] = (SEL_MIN if wd & Mn[i] else 0) | (SEL_MAX if wd & Mx[i] else 0) | (SEL_RANDOM if wd & Mr[i] else 0)
    return sel, chosen, sums


def _run_gpu(t: Dict[str, np.ndarray], times: Optional[dict] = None, keep: bool = False):
    import torch
    from . import engine
    d = {k: torch.from_numpy(np.ascontiguousarray(t[k])).cuda() for k in ("ring_xy", "ring_start", "ring_frame", "group", "cage", "cage_start", "area", "random_order")}
    bitmap = torch.zeros(int(t["bitmap_words"]), dtype=torch.int32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if times is not None else None
    if ev:
        ev[0].record()
    engine.dedup_fill(d["ring_xy"], d["ring_start"], d["ring_frame"], bitmap, t["ring_start"], t["ring_frame"])
    if ev:
        ev[1].record()
    words = engine.dedup_sets(d["group"], d["cage"], bitmap, t["group"])
    if ev:
        ev[2].record()
    sel, chosen, sums = engine.dedup_select(d["group"], d["cage_start"], d["cage"], words, d["area"], d["random_order"], t["group"], t["cage_start"])
    if ev:
        ev[3].record()
        ev[3].synchronize()
        for k, name in enumerate(("fill_ms", "sets_ms", "select_ms")):
            times[name] = times.get(name, 0.0) + ev[k].elapsed_time(ev[k + 1])
    host = lambda x: x.cpu().numpy().view(np.uint32) if keep else None      # (the bitmaps stay on the device unless a caller asks for them)
    return host(bitmap), host(words), sel.cpu().numpy(), chosen.cpu().numpy(), sums.cpu().numpy()


def _run_numpy(t: Dict[str, np.ndarray], times: Optional[dict] = None, keep: bool = False):
    import time
    t0 = time.perf_counter()
    bitmap = fill_numpy(t["ring_xy"], t["ring_start"], t["ring_frame"], t["bitmap_words"])
    t1 = time.perf_counter()
    words = sets_numpy(t["group"], t["cage"], bitmap)
    t2 = time.perf_counter()
    sel, chosen, sums = select_numpy(t["group"], t["cage_start"], t["cage"], words, t["area"], t["random_order"])
    if times is not None:
        for name, dt in (("fill_ms", t1 - t0), ("sets_ms", t2 - t1), ("select_ms", time.perf_counter() - t2)):
            times[name] = times.get(name, 0.0) + dt * 1e3
    return bitmap, words, sel, chosen, sums


def _selections(p: dict, run, budget: int, details: Optional[list], times: Optional[dict]) -> dict:
    G, C = len(p["slots"]), p["cage_group"].shape[0]
    bits, chosen, sums = np.zeros(C, np.uint8), np.zeros((G, 4), np.int32), np.zeros((G, MAX_PERMS), np.float64)
    for g0, g1 in chunks(p, budget):
        t = tables(p, g0, g1)
        bitmap, words, sel, ch, sm = run(t, times, details is not None)
        bits[t["rows"]], chosen[g0:g1], sums[g0:g1] = sel, ch, sm
        if details is not None:
            details.append({"groups": (g0, g1), "bitmap": bitmap, "words": words, "tables": t})
    return {"bits": bits, "chosen": chosen, "sums": sums}


def selections_gpu(p: dict, budget: int = BUDGET_BYTES, details: Optional[list] = None, times: Optional[dict] = None) -> dict:
    """The three launches per chunk of groups -> {"bits": uint8 [C] (SEL_* of the selections every cage survives), "chosen": int32 [G, 4]
    (the order numbers of min, max and random; n!), "sums": float64 [G, 120] (the area of every order)}.  details (a list) receives per
    chunk the bitmap, the words and the tables; times (a dict) the summed milliseconds of the launches (HIP events)."""
    return _selections(p, _run_gpu, budget, details, times)


def selections_numpy(p: dict, budget: int = BUDGET_BYTES, details: Optional[list] = None, times: Optional[dict] = None) -> dict:
    """selections_gpu's result from fill_numpy, sets_numpy and select_numpy: the same bytes."""
    return _selections(p, _run_numpy, budget, details, times)


def literal_mask(ring, w: int, h: int) -> np.ndarray:
    """bool [h, w]: the even-odd fill of a closed pixel ring, by counting: +1 at (r, x) for every unit edge of row r at x, a running sum
    along the row, odd = inside."""
    count = np.zeros((h, w + 1), np.int64)
    r = np.asarray(ring, np.int64).reshape(-1, 2)
    for (xa, ya), (xb, yb) in zip(r[:-1].tolist(), r[1:].tolist()):
        if xa == xb:
            count[min(ya, yb):max(ya, yb), xa] += 1
    return (np.cumsum(count, axis=1)[:, :w] % 2).astype(bool)


def selections_literal(p: dict) -> dict:
    """The reference's algorithm as it stands, slowly: per group and permutation the allotted regions mask_i & ~(everything before), a cage
    survives iff its window holds a pixel of its image's region; the area of the survivors per permutation; the reference's two
    comparisons; the problem's random order.  No set words: the yardstick for selections_numpy."""
    G, C = len(p["slots"]), p["cage_group"].shape[0]
    bits, chosen, sums = np.zeros(C, np.uint8), np.zeros((G, 4), np.int32), np.zeros((G, MAX_PERMS), np.float64)
    of_group: List[List[int]] = [[] for _ in range(G)]
    for e in range(C):
        if p["cage_group"][e] >= 0:
            of_group[int(p["cage_group"][e])].append(e)
    for g in range(G):
        w, h, n = int(p["w"][g]), int(p["h"][g]), len(p["slots"][g])
        masks = [np.ones((h, w), bool) if r is None else literal_mask(r, w, h) for r in p["slots"][g]]

        def survivors(perm):
            covered = np.zeros((h, w), bool)
            region = [None] * n
            for i in perm:
                region[i] = masks[i] & ~covered
                covered = covered | masks[i]
            alive = []
            for e in of_group[g]:
                i = int(p["cage_slot"][e])
                xmin, xmax, ymin, ymax = p["box"][e].tolist()
                if i >= 0 and region[i][max(ymin - 1, 0):max(min(ymax, h - 1) + 1, 0), max(xmin - 1, 0):max(min(xmax, w - 1) + 1, 0)].any():
                    alive.append(e)
            return alive

        best_max, best_min, out_max, out_min, qmax, qmin = 0.0, np.inf, [], [], -1, -1
        for q, perm in enumerate(itertools.permutations(range(n))):
            alive = survivors(perm)
            total = 0.0
            for e in alive:
                a = float(p["area"][e])
                total = total + (0.0 if a != a else a)
            sums[g, q] = total
            if total >= best_max:
                out_max, best_max, qmax = alive, total, q
            if total < best_min:
                out_min, best_min, qmin = alive, total, q
        order = tuple(int(j) for j in p["random_order"][g, :n])
        chosen[g] = (qmin, qmax, list(itertools.permutations(range(n))).index(order), _FACT[n])
        for alive, bit in ((out_min, SEL_MIN), (out_max, SEL_MAX), (survivors(order), SEL_RANDOM)):
            bits[alive] |= bit
    return {"bits": bits, "chosen": chosen, "sums": sums}


# ---- from a sweep's files to the problem ----

def read_blank_key(path: str) -> List[dict]:
    """The rows of image_boxes_blank_key.csv (blank.HEADER's columns)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    for c in ("image", "image_status"):
        if rows and c not in rows[0]:
            raise ValueError(f"{path}: no column {c!r} (the file of detect.py --blank-key)")
    return rows


def read_blank_geom(path: str) -> Dict[str, list]:
    """image (without its extension) -> ring_px of image_boxes_partly_blank.geojson."""
    with open(path) as f:
        feats = json.load(f)["features"]
    out = {}
    for ft in feats:
        pr = ft["properties"]
        if "ring_px" not in pr:
            raise ValueError(f"{path}: the feature of {pr.get('image')!r} has no ring_px (the file of detect.py --blank-geom)")
        out[_stem(pr["image"])] = pr["ring_px"]
    return out


def _stem(image: str) -> str:
    base = os.path.basename(image)
    for ext in (".jpeg", ".jpg", ".tif", ".tiff", ".png"):
        if base.lower().endswith(ext):
            return base[:-len(ext)]
    return base


def build_problem(table: Dict[str, np.ndarray], key_rows: Sequence[dict], rings: Dict[str, list], take: np.ndarray, areas: np.ndarray,
                  seed: int = 0, frame: int = FRAME) -> dict:
    """The problem of a sweep: groups = (image pass, bbox_ind, x_offset, y_offset) over the key's images that are complete, or partly blank
    with a ring; slots in ascending (year, image name); groups sorted by pass and tile key.  Cages = the rows of `table` with take[k], in
    row order, each on the slot of its image.  An image of the table that the key lacks is an error that lists the names.  The result
    also carries ``rows`` (the table row of every cage), ``images`` (per group, the slots' image names) and ``keys`` (pass, tile key)."""
    stems = [str(s) for s in table["stems"]]
    status = {}
    for r in key_rows:
        status[_stem(r["image"])] = r
    missing = sorted(s for s in set(stems) if s not in status)
    if missing:
        raise ValueError(f"dedup: {len(missing)} images of the label directory are not in the blank key: {' '.join(missing)}")
    members: Dict[Tuple[str, int, int, int], List[Tuple[int, str]]] = {}
    for stem, r in status.items():
        year, ind, xo, yo = aqblank.name_fields(stem)
        if ind == "":
            continue
        st = r["image_status"]
        if st == aqblank.COMPLETE or (st == aqblank.PARTLY_BLANK and stem in rings):
            members.setdefault((aqfac.image_pass(int(year)), int(ind), int(xo), int(yo)), []).append((int(year), stem))
    keys = sorted(members)
    slot_of: Dict[str, Tuple[int, int]] = {}
    slots, names, images, order = [], [], [], []
    for g, key in enumerate(keys):
        mem = sorted(members[key])
        names.append(f"pass {key[0]}, tile {key[1]}-{key[2]}-{key[3]} ({' '.join(s for _, s in mem)})")
        images.append([s for _, s in mem])
        slots.append([None if status[s]["image_status"] == aqblank.COMPLETE else rings[s] for _, s in mem])
        for j, (_, s) in enumerate(mem):
            slot_of[s] = (g, j)
        u = uniform(seed, key[1], key[2], key[3], np.asarray([y for y, _ in mem], np.uint64))
        by_u = sorted(range(len(mem)), key=lambda j: (float(u[j]), j))
        order.append((by_u + [-1] * MAX_SLOTS)[:MAX_SLOTS])
    rows = np.nonzero(np.asarray(take, bool))[0]
    where = np.asarray([slot_of.get(stems[int(i)], (-1, -1)) for i in table["image"][rows]], np.int64).reshape(-1, 2)
    box = np.stack([np.asarray(table[c], np.int64)[rows] for c in ("xmin", "xmax", "ymin", "ymax")], 1) if rows.shape[0] else np.zeros((0, 4), np.int64)
    G = len(keys)
    p = make_problem([frame] * G, [frame] * G, slots, where[:, 0], where[:, 1], box, np.asarray(areas, np.float64)[rows],
                     np.asarray(order, np.int32).reshape(-1, MAX_SLOTS), names)
    p.update(rows=rows, images=images, keys=[(k[0], f"{k[1]}-{k[2]}-{k[3]}") for k in keys])
    return p


def _durable(path: str, text: str) -> None:
    tmp = path + ".tmp"
    with open(tmp, "w", newline="") as f:
        f.write(text)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def write_files(out_dir: str, table, p: dict, res: dict, params: dict) -> None:
    """dedup_cages.csv, dedup_tiles.csv and dedup.json, each written to a temporary file, fsync'd and renamed; numbers by ``repr``."""
    os.makedirs(out_dir, exist_ok=True)
    stems = [str(s) for s in table["stems"]]
    lines = ["row,image,pass,tile_key,random,min,max\n"]
    for e, k in enumerate(p["rows"].tolist()):
        stem = stems[int(table["image"][k])]
        _, ind, xo, yo = aqblank.name_fields(stem)
        b = int(res["bits"][e])
        lines.append(f"{k},{stem}.jpeg,{aqfac.image_pass(int(table['year'][k]))},{ind}-{xo}-{yo},{int(bool(b & SEL_RANDOM))},{int(bool(b & SEL_MIN))},{int(bool(b & SEL_MAX))}\n")
    _durable(os.path.join(out_dir, CAGES_FILE), "".join(lines))
    lines = ["pass,tile_key,images,order_random,order_min,order_max,area_random,area_min,area_max\n"]
    for g, (ps, key) in enumerate(p["keys"]):
        n = int(p["n"][g])
        qmin, qmax, qr = (int(v) for v in res["chosen"][g, :3])
        text = lambda q: " ".join(str(j) for j in _PERMS[n][q]) if q >= 0 else ""
        val = lambda q: repr(float(res["sums"][g, q])) if q >= 0 else ""
        lines.append(f"{ps},{key},{' '.join(p['images'][g])},{text(qr)},{text(qmin)},{text(qmax)},{val(qr)},{val(qmin)},{val(qmax)}\n")
    _durable(os.path.join(out_dir, TILES_FILE), "".join(lines))
    _durable(os.path.join(out_dir, JSON_FILE), json.dumps(params, indent=1) + "\n")


def dedup_from_table(table: Dict[str, np.ndarray], blank_key: str, blank_geom: str, out_dir: Optional[str] = None, selection: str = "random",
                     seed: int = 0, conf_thresh: float = 0.5, keep=None, widths=geocode.IM_WIDTH, heights=geocode.IM_HEIGHT,
                     cpu: bool = False) -> dict:
    """The whole step on a geocoded table: the detections with det_conf >= conf_thresh (and keep[k]: the land filter's ocean rows) take
    part, as the reference filters ``preds`` before de-duplicating.  -> {"bits": uint8 per table row (0 for a row that takes no part),
    "take", "selection", "problem", "result"}; with out_dir the three files."""
    if selection not in SELECTIONS:
        raise ValueError(f"dedup: selection {selection!r} (random, min or max)")
    n_all = np.asarray(table["det_conf"]).shape[0]
    take = np.asarray(table["det_conf"], np.float64) >= conf_thresh
    if keep is not None:
        take &= np.asarray(keep, bool)
    areas = aqfac.net_areas(table, widths, heights)["area"]
    p = build_problem(table, read_blank_key(blank_key), read_blank_geom(blank_geom), take, areas, seed)
    res = (selections_numpy if cpu else selections_gpu)(p)
    bits = np.zeros(n_all, np.uint8)
    bits[p["rows"]] = res["bits"]
    device = "cpu"
    if not cpu:
        import torch
        device = torch.cuda.get_device_name(0)
    if out_dir is not None:
        counts = {name: int(((res["bits"] & bit) != 0).sum()) for name, bit in SELECTIONS.items()}
        write_files(out_dir, table, p, res, {"device": device, "cpu": bool(cpu), "selection": selection, "seed": int(seed), "facilities_conf": float(conf_thresh),
                                             "land_filter": keep is not None, "frame": FRAME, "detections": int(n_all), "cages": int(p["rows"].shape[0]),
                                             "groups": len(p["slots"]), "images_in_groups": int(p["n"].sum()),
                                             "cages_without_image": int((p["cage_group"] < 0).sum()), "survivors": counts})
    return {"bits": bits, "take": take, "selection": selection, "problem": p, "result": res}


def survivors(dd: dict, selection: Optional[str] = None) -> np.ndarray:
    """bool per table row: takes part and survives the selection (default: the run's own)."""
    return dd["take"] & ((dd["bits"] & SELECTIONS[selection or dd["selection"]]) != 0)


def describe(dd: dict) -> str:
    p, b = dd["problem"], dd["result"]["bits"]
    return (f"{p['rows'].shape[0]} cages on {int(p['n'].sum())} images of {len(p['slots'])} tiles: " +
            ", ".join(f"{name} keeps {int(((b & bit) != 0).sum())}" for name, bit in SELECTIONS.items()))


# ---- cage_ids_min / cage_ids_max (reference compute_min_max_cages, :997-1064) ----

def _boxes(table, ids: Sequence[int]) -> np.ndarray:
    """float64 [m, 4] (x0, y0, x1, y1) in EPSG:3857: the circle and square cages among `ids` (the reference's all_cages)."""
    cls = np.asarray(table["cls"], np.int64)
    ids = [i for i in ids if cls[i] in (aqfac.CLS_OF["circle_farm"], aqfac.CLS_OF["square_farm"])]
    return np.stack([np.asarray(table[c], np.float64)[ids] for c in ("xmin_3857", "ymin_3857", "xmax_3857", "ymax_3857")], 1) if ids else np.zeros((0, 4))


def union_overlap(a: np.ndarray, b: np.ndarray) -> Optional[float]:
    """area(U(a) & U(b)) / area(U(a)) for two sets of closed boxes [m, 4] (x0, y0, x1, y1), on the compressed coordinate grid of both;
    None if no box of a intersects a box of b (touching counts, as sjoin's ``intersects``); 0.0 if U(a) has no area."""
    if a.shape[0] == 0 or b.shape[0] == 0:
        return None
    hit = (a[:, None, 0] <= b[None, :, 2]) & (b[None, :, 0] <= a[:, None, 2]) & (a[:, None, 1] <= b[None, :, 3]) & (b[None, :, 1] <= a[:, None, 3])
    if not hit.any():
        return None
    xs, ys = np.unique(np.concatenate([a[:, [0, 2]].ravel(), b[:, [0, 2]].ravel()])), np.unique(np.concatenate([a[:, [1, 3]].ravel(), b[:, [1, 3]].ravel()]))

    def cover(boxes):
        m = np.zeros((ys.shape[0] - 1, xs.shape[0] - 1), bool)
        for x0, y0, x1, y1 in boxes.tolist():
            m[np.searchsorted(ys, y0):np.searchsorted(ys, y1), np.searchsorted(xs, x0):np.searchsorted(xs, x1)] = True
        return m
    cell = np.diff(ys)[:, None] * np.diff(xs)[None, :]
    ca, cb = cover(a), cover(b)
    whole = float(cell[ca].sum())
    return float(cell[ca & cb].sum()) / whole if whole > 0 else 0.0


def match_cage_ids(table, fac: Dict[str, list], other: Dict[str, list]) -> List[Optional[List[int]]]:
    """For every facility of `fac`: the cage_ids of the same-pass facility of `other` whose circle and square cages intersect its own with
    the largest overlap (ties: the smallest facility_index); None without one."""
    theirs = [_boxes(table, ids) for ids in other["cage_ids"]]
    out: List[Optional[List[int]]] = []
    for f in range(len(fac["facility_index"])):
        mine = _boxes(table, fac["cage_ids"][f])
        best, at = -1.0, None
        for o in range(len(other["facility_index"])):
            if other["pass"][o] != fac["pass"][f]:
                continue
            v = union_overlap(mine, theirs[o])
            if v is not None and v > best:
                best, at = v, o
        out.append(None if at is None else list(other["cage_ids"][at]))
    return out


def cluster(table, dd: dict, conf_thresh: float = 0.5, eps: float = 10.0, min_cages: int = 5, widths=geocode.IM_WIDTH, heights=geocode.IM_HEIGHT,
            labels_fn=None) -> Dict[str, list]:
    """facilities.cluster by pass on the survivors of the run's selection, with the columns cage_ids_min / cage_ids_max from the clusterings
    of the min and max survivors: no match under min gives [] (the reference's fillna), under max the facility's own cage_ids."""
    run = lambda sel: aqfac.cluster(table, "pass", conf_thresh, eps, min_cages, widths, heights, labels_fn=labels_fn, keep=survivors(dd, sel))
    fac = run(dd["selection"])
    for sel in ("min", "max"):
        matched = match_cage_ids(table, fac, fac if sel == dd["selection"] else run(sel))
        fac[f"cage_ids_{sel}"] = [([] if sel == "min" else list(own)) if m is None else m for m, own in zip(matched, fac["cage_ids"])]
    return fac


# ---- command line ----

def add_options(p: argparse.ArgumentParser) -> None:
    """The options detect.py and this module's command line share."""
    p.add_argument("--dedup-selection", choices=tuple(SELECTIONS), default="random",
                   help="which order of a tile's years decides: a seeded shuffle (the reference's default), or the order with the smallest / largest cage area")
    p.add_argument("--dedup-seed", type=int, default=0, metavar="SEED", help="64-bit seed of the random selection (the Philox key)")


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.dedup",
                                description="Keep one year's cages per tile and image pass for an existing label directory, without running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv")
    p.add_argument("--blank-key", required=True, metavar="CSV", help="image_boxes_blank_key.csv of detect.py --blank-key")
    p.add_argument("--blank-geom", required=True, metavar="GEOJSON", help="image_boxes_partly_blank.geojson of detect.py --blank-geom")
    p.add_argument("--out", default=None, metavar="DIR", help="default <labels>/..")
    p.add_argument("--land", default=None, metavar="GEOJSON", help="land polygons: only the detections at sea take part (the --land-filter step)")
    p.add_argument("--facilities-conf", type=float, default=0.5, metavar="CONF", help="detections with det_conf >= CONF take part")
    p.add_argument("--image-size", nargs=2, type=int, default=[geocode.IM_WIDTH, geocode.IM_HEIGHT], metavar=("W", "H"),
                   help="pixel size of the images (the border test of the circle areas)")
    p.add_argument("--cpu", action="store_true", help="the numpy restatement instead of the GPU (the same bytes)")
    add_options(p)
    opt = p.parse_args(argv)
    out = opt.out or os.path.dirname(os.path.abspath(opt.labels.rstrip("/")))
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    keep = None
    if opt.land:
        from . import land as aqland
        keep = aqland.ocean_rows(table, aqland.load_land_geojson(opt.land), cpu=opt.cpu)
    dd = dedup_from_table(table, opt.blank_key, opt.blank_geom, out, opt.dedup_selection, opt.dedup_seed, opt.facilities_conf, keep,
                          opt.image_size[0], opt.image_size[1], cpu=opt.cpu)
    print(f"{describe(dd)} in {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
