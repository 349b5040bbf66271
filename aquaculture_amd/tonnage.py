"""Live-weight production of the facilities per image pass (``detect.py --tonnage``, ``python -m aquaculture_amd.tonnage``).

The reference's measuring step (src/utils_tonnage.py:28-127, compute_facility_tonnage_estimates, with :330-458, sample_model_errors): a
Monte-Carlo bootstrap of K simulations.  In each one every cage of every facility gets a model error added to its area estimate (drawn again
while the area is not positive), the facility's area is drawn uniformly between the sum of the cages' lower bounds and the sum of their
upper bounds, its cage depth from a mixture of two truncated normals, the pass's stocking density from a truncated normal and its harvest
frequency from a normal; tonnes = area x depth x stocking x harvest / 1000, summed per pass.  The table returned is the reference's: mean,
variance and standard deviation of the K pass sums.

The simulation runs on the GPU (csrc/tonnage.hip through engine.tonnage_simulate) or, with cpu=True, in simulate_numpy; both give the
same bytes, because the generator is counter-based (Philox4x32-10; a draw depends only on seed, simulation, entity, slot and attempt) and
every floating-point step is one of + - x / sqrt, in one written order (include/aq_engine.h).  The inverse normal distribution function is
the Cephes Math Library's ndtri with an arithmetic-only logarithm.

Departures from the reference, all stated in DESIGN.md section 17: the random stream is not numpy's (the distributions are; pinned by
tests/test_tonnage.py); a cage whose area stays non-positive for 64 draws keeps its original area (the reference draws for ever); a
facility whose cage depth is not above the minimum depth gets the minimum depth (the reference divides 0 by 0); the truncated normals are
drawn by inversion, as scipy does; cages without an area estimate (neither circle nor square) take no part, as pandas' sums skip their NaN.
"""
from __future__ import annotations

import argparse
import csv
import json
import math
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import facilities as aqfac
from . import geocode

SLOT_ERROR, SLOT_AREA, SLOT_BERNOULLI, SLOT_DEPTH_A, SLOT_DEPTH_B, SLOT_STOCKING, SLOT_HARVEST = range(7)
MAX_ATTEMPTS = 64
KIND_FULL, KIND_BORDER, KIND_SQUARE = 0, 1, 2
SEL_MIN, SEL_MAX, SEL_RANDOM = 4, 8, 16
STOCKING_BOUNDS = (5.0, 20.0)                               # reference utils_tonnage.py:96
DEFAULT_DEPTH, DEFAULT_MIN_DEPTH = 4.84, 1.0                # the reference README's values
TON_BUDGET_BYTES = 256 << 20                                # of ton [K_chunk, F] per call

_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
LN2 = 0.6931471805599453
EXPM2 = 0.13533528323661269189
S2PI = 2.50662827463100050242E0
TWO_PLUS_PI = 2.0 + 3.141592653589793
TWO_PI = 2.0 * 3.141592653589793

# The coefficient tables of the Cephes Math Library's ndtri (Stephen L. Moshier; 3-clause BSD), leading coefficient first.
_P0 = (-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1, 1.39312609387279679503E1, -1.23916583867381258016E0)
_Q0 = (1.00000000000000000000E0, 1.95448858338141759834E0, 4.67627912898881538453E0, 8.63602421390890590575E1, -2.25462687854119370527E2,
       2.00260212380060660359E2, -8.20372256168333339912E1, 1.59056225126211695515E1, -1.18331621121330003142E0)
_P1 = (4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1, 4.40805073893200834700E1, 1.46849561928858024014E1,
       2.18663306850790267539E0, -1.40256079171354495875E-1, -3.50424626827848203418E-2, -8.57456785154685413611E-4)
_Q1 = (1.00000000000000000000E0, 1.57799883256466749731E1, 4.53907635128879210584E1, 4.13172038254672030440E1, 1.50425385692907503408E1,
       2.50464946208309415979E0, -1.42182922854787788574E-1, -3.80806407691578277194E-2, -9.33259480895457427372E-4)
_P2 = (3.23774891776946035970E0, 6.91522889068984211695E0, 3.93881025292474443415E0, 1.33303460815807542389E0, 2.01485389549179081538E-1,
       1.23716634817820021358E-2, 3.01581553508235416007E-4, 2.65806974686737550832E-6, 6.23974539184983293730E-9)
_Q2 = (1.00000000000000000000E0, 6.02427039364742014255E0, 3.67983563856160859403E0, 1.37702099489081330271E0, 2.16236993594496635890E-1,
       1.34204006088543189037E-2, 3.28014464682127739104E-4, 2.89247864745380683936E-6, 6.79019408009981274425E-9)


# ---- the restatement's building blocks (the operation order of csrc/tonnage.hip's head comment) ----

def philox4x32(c0, c1, c2, c3, key0: int, key1: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Philox4x32-10 on arrays of counter words (each < 2^32, any broadcastable shapes) -> the four output words, uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & _MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(key0 & 0xFFFFFFFF), np.uint64(key1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                         # 32 x 32 bits: the product fits 64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniform_from_words(w0, w1) -> np.ndarray:
    x = ((np.asarray(w1, np.uint64) << _S32) | np.asarray(w0, np.uint64)) >> np.uint64(11)
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -53
    return np.where(u < 1.0, u, 1.0 - 2.0 ** -53)


def uniform(seed: int, k, entity, slot, attempt) -> np.ndarray:
    """The draw of counter (k, entity, slot, attempt) under `seed` (key words: its low and high half), strictly inside (0, 1)."""
    w0, w1, _, _ = philox4x32(k, entity, slot, attempt, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return uniform_from_words(w0, w1)


def alog(x) -> np.ndarray:
    """ln x for positive finite x in + - x / only."""
    m, e = np.frexp(np.asarray(x, np.float64))              # x = m 2^e, 0.5 <= m < 1
    lo = m < 0.7071067811865476
    m = np.where(lo, m * 2.0, m)
    e = np.where(lo, e - 1, e)
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    acc = np.full_like(s, 1.0 / 27.0)
    for j in range(25, 0, -2):
        acc = acc * s2 + 1.0 / j
    return e.astype(np.float64) * LN2 + (2.0 * s) * acc


def _horner(x, c):
    r = np.full_like(x, c[0])
    for v in c[1:]:
        r = r * x + v
    return r


def ndtri(p) -> np.ndarray:
    p = np.asarray(p, np.float64)
    shape = p.shape
    p = p.reshape(-1)
    out = np.full(p.shape, np.nan)
    with np.errstate(all="ignore"):
        ok = (p >= 0.0) & (p <= 1.0)
        out[ok & (p == 0.0)] = -np.inf
        out[ok & (p == 1.0)] = np.inf
        ok &= (p != 0.0) & (p != 1.0)
        mirrored = p > 1.0 - EXPM2
        y = np.where(mirrored, 1.0 - p, p)
        central = ok & (y > EXPM2)
        yc = y[central] - 0.5
        y2 = yc * yc
        out[central] = (yc + yc * ((y2 * _horner(y2, _P0)) / _horner(y2, _Q0))) * S2PI
        tail = ok & ~central
        yt = y[tail]
        x = np.sqrt(-2.0 * alog(yt))
        x0 = x - alog(x) / x
        z = 1.0 / x
        x1 = np.where(x < 8.0, (z * _horner(z, _P1)) / _horner(z, _Q1), (z * _horner(z, _P2)) / _horner(z, _Q2))
        r = x0 - x1
        out[tail] = np.where(mirrored[tail], r, -r)
    return out.reshape(shape)


# ---- the simulation table ----

def depth_probs() -> np.ndarray:
    """Phi(-1.96), Phi(0), Phi(0), Phi(1.96): the bounds of the two truncated normals of the depth, as probabilities."""
    from scipy.special import ndtr
    return np.asarray(ndtr(np.array([-1.96, 0.0, 0.0, 1.96])), np.float64)


def pass_params(s_mean, s_sd, h_mean, h_sd) -> np.ndarray:
    """float64 [P, 6]: s_mean, s_sd, pS0, pS1, h_mean, h_sd with pS0, pS1 = Phi((5 - s_mean) / s_sd), Phi((20 - s_mean) / s_sd)."""
    from scipy.special import ndtr
    s_mean, s_sd, h_mean, h_sd = (np.asarray(v, np.float64).reshape(-1) for v in (s_mean, s_sd, h_mean, h_sd))
    if not (np.isfinite(s_mean).all() and np.isfinite(s_sd).all() and np.isfinite(h_mean).all() and np.isfinite(h_sd).all()):
        raise ValueError("tonnage: a factor that is not finite")
    if (s_sd <= 0).any():
        raise ValueError("tonnage: s_sd has to be positive")
    return np.ascontiguousarray(np.stack([s_mean, s_sd, ndtr((STOCKING_BOUNDS[0] - s_mean) / s_sd), ndtr((STOCKING_BOUNDS[1] - s_mean) / s_sd),
                                          h_mean, h_sd], 1))


def make_table(entry_start, area, err_mean, err_sd, kind, sel, depth, pass_id, params, mix: float = 0.5, min_depth: float = DEFAULT_MIN_DEPTH) -> dict:
    """The arrays both paths take.  entry_start [F + 1]: facility f owns entries entry_start[f] .. entry_start[f + 1] - 1; per entry area
    (area_orig), err_mean, err_sd, kind (KIND_*), sel (SEL_MIN | SEL_MAX | SEL_RANDOM bits); per facility depth (cage_depth) and
    pass_id (row of params = pass_params(...))."""
    t = {"entry_start": np.ascontiguousarray(entry_start, dtype=np.int32), "area": np.ascontiguousarray(area, dtype=np.float64),
         "err": np.ascontiguousarray(np.stack([np.asarray(err_mean, np.float64), np.asarray(err_sd, np.float64)], 1)),
         "flags": np.ascontiguousarray((np.asarray(kind, np.int64) & 3) | np.asarray(sel, np.int64), dtype=np.uint8),
         "depth": np.ascontiguousarray(depth, dtype=np.float64), "pass_id": np.ascontiguousarray(pass_id, dtype=np.int32),
         "params": np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 6), "mix": float(mix), "min_depth": float(min_depth),
         "probs": depth_probs()}
    F, E = t["depth"].shape[0], t["area"].shape[0]
    st = t["entry_start"]
    if st.shape != (F + 1,) or t["pass_id"].shape != (F,) or t["err"].shape != (E, 2) or t["flags"].shape != (E,):
        raise ValueError("tonnage: the table's arrays do not fit each other")
    if F and (st[0] < 0 or st[-1] > E or (np.diff(st) < 0).any()):
        raise ValueError("tonnage: entry offsets have to be non-decreasing inside the entries")
    if not 0.0 <= t["mix"] <= 1.0 or not math.isfinite(t["min_depth"]):
        raise ValueError(f"tonnage: mix = {mix} (a probability), min_depth = {min_depth}")
    if F and (t["params"].shape[0] < 1 or not np.isfinite(t["params"]).all() or (t["params"][:, 1] <= 0).any()):
        raise ValueError("tonnage: pass parameters have to be finite, s_sd positive, and at least one pass given")
    return t


# ---- the restatement ----

def simulate_numpy(t: dict, K: int, seed: int = 0, k0: int = 0, stats: Optional[dict] = None) -> np.ndarray:
    """ton float64 [K, F] of simulations k0 .. k0 + K - 1, as csrc/tonnage.hip computes it: a loop over the entry position inside a
    facility, whole (k, f) planes at a time, so that lo and hi are the same sequential sums.  stats (a dict) receives ``draws``: how many
    (simulation, entry) pairs needed at least a-th extra draw, per a (a list); ``capped``; ``min_area``: the smallest accepted area;
    ``lo`` / ``hi`` [K, F]."""
    F = t["depth"].shape[0]
    K = int(K)
    if k0 < 0 or k0 + K > 1 << 32:
        raise ValueError(f"tonnage: simulations {k0} .. {k0 + K} (the counter's word holds 0 .. 2^32 - 1)")
    E, P = t["area"].shape[0], t["params"].shape[0]
    ks = (np.arange(K, dtype=np.uint64) + np.uint64(k0))[:, None]
    start = np.minimum(np.maximum(t["entry_start"].astype(np.int64), 0), E)
    first, end = start[:-1], np.minimum(np.maximum(start[1:], start[:-1]), E)
    lo, hi = np.zeros((K, F)), np.zeros((K, F))
    extra = [0] * MAX_ATTEMPTS
    capped, min_area = 0, np.inf
    with np.errstate(all="ignore"):
        for j in range(int((end - first).max()) if F else 0):
            fs = np.nonzero(end - first > j)[0]
            e = first[fs] + j
            a0, mean, sd, fl = t["area"][e][None, :], t["err"][e, 0][None, :], t["err"][e, 1][None, :], t["flags"][e].astype(np.int64)
            a = np.broadcast_to(a0, (K, fs.shape[0])).copy()
            todo = np.ones(a.shape, bool)
            for attempt in range(MAX_ATTEMPTS):
                kk, ee = np.nonzero(todo)
                if kk.shape[0] == 0:
                    break
                if attempt:
                    extra[attempt - 1] += kk.shape[0]
                u = uniform(seed, ks[kk, 0], e[ee].astype(np.uint64), SLOT_ERROR, attempt)
                v = a0[0, ee] + (mean[0, ee] + sd[0, ee] * ndtri(u))
                a[kk, ee] = v
                todo[kk, ee] = v <= 0.0
            capped += int(todo.sum())
            a = np.where(todo, np.broadcast_to(a0, a.shape), a)
            if a.size:
                min_area = min(min_area, float(np.nanmin(a))) if not np.isnan(a).all() else min_area
            kind = (fl & 3)[None, :]
            mn = np.where(kind == KIND_BORDER, (4.0 * a) / TWO_PLUS_PI, np.where(kind == KIND_SQUARE, (2.0 * a) / 3.0, a))
            mx = np.where(kind == KIND_BORDER, (TWO_PI * a) / TWO_PLUS_PI, np.where(kind == KIND_SQUARE, (4.0 * a) / 3.0, a))
            lo[:, fs] = np.where((fl & SEL_MIN)[None, :] != 0, lo[:, fs] + mn, lo[:, fs])
            hi[:, fs] = np.where((fl & SEL_MAX)[None, :] != 0, hi[:, fs] + mx, hi[:, fs])
        if stats is not None:
            stats.update(draws=extra, capped=capped, min_area=min_area, lo=lo, hi=hi)
        if F == 0 or K == 0:
            return np.zeros((K, F))
        fe = np.arange(F, dtype=np.uint64)[None, :]
        sim_area = lo + (hi - lo) * uniform(seed, ks, fe, SLOT_AREA, 0)
        d, m = t["depth"][None, :], t["min_depth"]
        pA0, pA1, pB0, pB1 = (float(v) for v in t["probs"])
        use_a = uniform(seed, ks, fe, SLOT_BERNOULLI, 0) < t["mix"]
        dA = d + ((d - m) / 1.96) * ndtri(pA0 + uniform(seed, ks, fe, SLOT_DEPTH_A, 0) * (pA1 - pA0))
        dB = d + (d / 1.96) * ndtri(pB0 + uniform(seed, ks, fe, SLOT_DEPTH_B, 0) * (pB1 - pB0))
        depth = np.where(d > m, np.where(use_a, dA, dB), m)
        q = t["params"][np.minimum(np.maximum(t["pass_id"], 0), P - 1)]
        stocking = q[:, 0][None, :] + q[:, 1][None, :] * ndtri(q[:, 2][None, :] + uniform(seed, ks, fe, SLOT_STOCKING, 0) * (q[:, 3] - q[:, 2])[None, :])
        harvest = q[:, 4][None, :] + q[:, 5][None, :] * ndtri(uniform(seed, ks, fe, SLOT_HARVEST, 0))
        return ((sim_area * depth) * stocking) * (harvest * (1 / 1000))


def reduce_numpy(ton: np.ndarray, pass_id, P: int, moments: np.ndarray) -> np.ndarray:
    """T [K, P] = the pass sums in ascending f; moments [F, 2] grows by the sums and sums of squares in ascending k.  Plain loops: numpy's
    own reductions add pairwise."""
    K, F = ton.shape
    T = np.zeros((K, P))
    with np.errstate(all="ignore"):
        for f in range(F):
            if 0 <= pass_id[f] < P:
                T[:, pass_id[f]] = T[:, pass_id[f]] + ton[:, f]
        for k in range(K):
            moments[:, 0] = moments[:, 0] + ton[k]
            moments[:, 1] = moments[:, 1] + ton[k] * ton[k]
    return T


def chunk_sizes(K: int, F: int, chunk: Optional[int] = None, budget: int = TON_BUDGET_BYTES) -> List[int]:
    if chunk is None:
        chunk = max(1, min(budget // (8 * max(F, 1)), (1 << 31) - 1))
    return [min(chunk, K - a) for a in range(0, K, chunk)]


def simulate(t: dict, K: int, seed: int = 0, k0: int = 0, cpu: bool = False, chunk: Optional[int] = None, keep_ton: bool = False) -> dict:
    """K simulations from k0 in chunks that keep ton under a memory budget (or `chunk` rows) -> {"T": [K, P], "moments": [F, 2] (sum and
    sum of squares over the simulations), "ton": [K, F] with keep_ton}.  cpu: simulate_numpy / reduce_numpy; else the GPU.  The split into
    chunks changes no byte."""
    F, P = t["depth"].shape[0], t["params"].shape[0]
    sizes = chunk_sizes(int(K), F, chunk if chunk is not None else (512 if cpu else None))
    Ts, tons = [], []
    if cpu:
        moments = np.zeros((F, 2))
        at = int(k0)
        for n in sizes:
            ton = simulate_numpy(t, n, seed, at)
            Ts.append(reduce_numpy(ton, t["pass_id"], P, moments))
            if keep_ton:
                tons.append(ton)
            at += n
    else:
        import torch
        from . import engine
        dev = {k: torch.from_numpy(t[k]).cuda() for k in ("entry_start", "area", "err", "flags", "depth", "pass_id", "params")}
        mom = torch.zeros((F, 2), dtype=torch.float64, device="cuda")
        at = int(k0)
        for n in sizes:
            ton, T = engine.tonnage_simulate(seed, at, n, dev["entry_start"], dev["area"], dev["err"], dev["flags"], dev["depth"], dev["pass_id"],
                                             dev["params"], t["mix"], t["min_depth"], t["probs"], mom, t["entry_start"], t["params"])
            Ts.append(T.cpu().numpy())
            if keep_ton:
                tons.append(ton.cpu().numpy())
            at += n
        moments = mom.cpu().numpy()
    out = {"T": np.concatenate(Ts, 0) if Ts else np.zeros((0, P)), "moments": moments}
    if keep_ton:
        out["ton"] = np.concatenate(tons, 0) if tons else np.zeros((0, F))
    return out


# ---- inputs the reference keeps in its own files ----

def _records(path: str, columns: Sequence[str]) -> List[dict]:
    """Rows of a CSV (with a header) or a JSON list of objects; every one of `columns` has to be there."""
    if path.lower().endswith(".json"):
        rows = json.load(open(path))
        if not isinstance(rows, list) or not all(isinstance(r, dict) for r in rows):
            raise ValueError(f"{path}: a JSON list of objects is expected")
    else:
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
    for i, r in enumerate(rows):
        missing = [c for c in columns if c not in r or r[c] is None or r[c] == ""]
        if missing:
            raise ValueError(f"{path}: row {i + 1} lacks {', '.join(missing)} (columns: {', '.join(columns)})")
    return rows


def _finite(path: str, row: int, name: str, v) -> float:
    try:
        x = float(v)
    except (TypeError, ValueError):
        x = math.nan
    if not math.isfinite(x):
        raise ValueError(f"{path}: row {row}: {name} = {v!r} is not a finite number")
    return x


def read_factors(path: str) -> Dict[str, Tuple[float, float, float, float]]:
    """--tonnage-factors: pass -> (s_mean, s_sd, h_mean, h_sd); the columns the reference renames at src/Results/tonnage_estimates.py:347-354."""
    out: Dict[str, Tuple[float, float, float, float]] = {}
    rows = _records(path, ("pass", "s_mean", "s_sd", "h_mean", "h_sd"))
    if not rows:
        raise ValueError(f"{path}: no pass")
    for i, r in enumerate(rows):
        v = tuple(_finite(path, i + 1, c, r[c]) for c in ("s_mean", "s_sd", "h_mean", "h_sd"))
        if v[1] <= 0:
            raise ValueError(f"{path}: row {i + 1}: s_sd = {v[1]} has to be positive")
        if v[3] < 0:
            raise ValueError(f"{path}: row {i + 1}: h_sd = {v[3]} is negative")
        if str(r["pass"]) in out:
            raise ValueError(f"{path}: pass {r['pass']} is listed twice")
        out[str(r["pass"])] = v
    return out


def read_errors(path: str) -> Dict[Tuple[str, str], Tuple[float, float]]:
    """--tonnage-errors: (pass, farm_type) -> (model_error_mean, model_error_sd); farm_type circle_farm or square_farm."""
    out: Dict[Tuple[str, str], Tuple[float, float]] = {}
    for i, r in enumerate(_records(path, ("pass", "farm_type", "model_error_mean", "model_error_sd"))):
        key = (str(r["pass"]), str(r["farm_type"]))
        if key[1] not in ("circle_farm", "square_farm"):
            raise ValueError(f"{path}: row {i + 1}: farm_type {key[1]!r} (circle_farm or square_farm)")
        v = (_finite(path, i + 1, "model_error_mean", r["model_error_mean"]), _finite(path, i + 1, "model_error_sd", r["model_error_sd"]))
        if v[1] < 0:
            raise ValueError(f"{path}: row {i + 1}: model_error_sd = {v[1]} is negative")
        if key in out:
            raise ValueError(f"{path}: {key[0]} / {key[1]} is listed twice")
        out[key] = v
    return out


def read_depths(path: str) -> Dict[int, float]:
    """--tonnage-depths: facility_index -> cage_depth (metres)."""
    out: Dict[int, float] = {}
    for i, r in enumerate(_records(path, ("facility_index", "cage_depth"))):
        try:
            fi = int(r["facility_index"])
        except (TypeError, ValueError):
            raise ValueError(f"{path}: row {i + 1}: facility_index = {r['facility_index']!r}") from None
        if fi in out:
            raise ValueError(f"{path}: facility {fi} is listed twice")
        out[fi] = _finite(path, i + 1, "cage_depth", r["cage_depth"])
    return out


# ---- from the facility table to the estimates ----

def build_table(fac: Dict[str, list], areas: Optional[Dict[str, np.ndarray]], table: Dict[str, np.ndarray], factors, errors=None, depths=None,
                mix: float = 0.5, min_depth: float = DEFAULT_MIN_DEPTH, default_depth: float = DEFAULT_DEPTH) -> Tuple[dict, List[str]]:
    """(make_table(...), the passes in sorted order) from cluster(table, "pass")'s result.  A facility's entries are the cages of its
    cage_ids, cage_ids_min and cage_ids_max (the last two default to cage_ids) in ascending cage id, as the reference's pivot orders
    them, each with the bits of the selections it is in; a cage without an area estimate is left out.  The model error of a cage is that
    of (its own year's pass, its type); none listed: (0, 0), the reference's table for human labels."""
    if "pass" not in fac:
        raise ValueError("tonnage: the facilities have to be clustered by pass")
    areas = fac["_areas"] if areas is None else areas
    errors = errors or {}
    depths = depths or {}
    F = len(fac["facility_index"])
    passes = sorted(set(fac["pass"]))
    lacking = [p for p in passes if p not in factors]
    if lacking:
        raise ValueError(f"tonnage: no factors for pass {', '.join(map(str, lacking))}")
    circle, square = aqfac.CLS_OF["circle_farm"], aqfac.CLS_OF["square_farm"]
    cls, years = np.asarray(table["cls"], np.int64), np.asarray(table["year"], np.int64)
    start, ids, sel = [0], [], []
    for f in range(F):
        member: Dict[int, int] = {}
        for col, bit in (("cage_ids_min", SEL_MIN), ("cage_ids_max", SEL_MAX), ("cage_ids", SEL_RANDOM)):
            for c in fac[col][f] if col in fac else fac["cage_ids"][f]:
                member[int(c)] = member.get(int(c), 0) | bit
        for c in sorted(member):
            if cls[c] in (circle, square) and not np.isnan(areas["area"][c]):
                ids.append(c)
                sel.append(member[c])
        start.append(len(ids))
    ids_a = np.asarray(ids, np.int64)
    kind = np.where(cls[ids_a] == square, KIND_SQUARE, np.where(np.asarray(areas["area_var"])[ids_a] == 0.0, KIND_FULL, KIND_BORDER))
    err = np.zeros((ids_a.shape[0], 2))
    for i, c in enumerate(ids):
        err[i] = errors.get((aqfac.image_pass(int(years[c])), geocode.REVERSE_CLASS_MAPPING[int(cls[c])]), (0.0, 0.0))
    depth = np.asarray([max(float(depths.get(int(fi), default_depth)), float(min_depth)) for fi in fac["facility_index"]], np.float64)
    params = pass_params(*([factors[p][j] for p in passes] for j in range(4))) if passes else np.zeros((0, 6))
    t = make_table(start, np.asarray(areas["area"], np.float64)[ids_a], err[:, 0], err[:, 1], kind, sel, depth,
                   [passes.index(p) for p in fac["pass"]], params, mix, min_depth)
    t["cage_ids"] = ids_a
    return t, passes


def estimate(fac, areas, table, factors, errors=None, depths=None, K: int = 10000, seed: int = 0, mix: float = 0.5,
             min_depth: float = DEFAULT_MIN_DEPTH, cpu: bool = False, default_depth: float = DEFAULT_DEPTH) -> dict:
    """The per-pass table of the reference's compute_facility_tonnage_estimates -- pass, tonnage, tonnage_var, tonnage_sd: np.mean, np.var and
    its root over the K pass sums, sorted by pass -- and, beside the reference's, per facility tonnage (mean) and tonnage_sd over the K
    simulations, from the sum and the sum of squares."""
    if K < 1:
        raise ValueError(f"tonnage: K = {K} simulations")
    t, passes = build_table(fac, areas, table, factors, errors, depths, mix, min_depth, default_depth)
    res = simulate(t, K, seed, cpu=cpu)
    T, mom = res["T"], res["moments"]
    mean = [float(np.mean(T[:, p])) for p in range(len(passes))]
    var = [float(np.var(T[:, p])) for p in range(len(passes))]
    f_mean = mom[:, 0] / K
    f_var = np.maximum(mom[:, 1] / K - f_mean * f_mean, 0.0)
    return {"pass": passes, "tonnage": mean, "tonnage_var": var, "tonnage_sd": [float(np.sqrt(v)) for v in var],
            "facility_index": [int(i) for i in fac["facility_index"]], "facility_pass": list(fac["pass"]),
            "facility_tonnage": [float(v) for v in f_mean], "facility_tonnage_sd": [float(v) for v in np.sqrt(f_var)],
            "facility_cages": np.diff(t["entry_start"]).tolist(), "T": T, "K": int(K), "seed": int(seed)}


ESTIMATES_FILE, FACILITIES_FILE, JSON_FILE = "tonnage_estimates.csv", "tonnage_facilities.csv", "tonnage.json"


def write_files(out_dir: str, est: dict, params: dict, more_rows: Sequence[Tuple[str, str, float, float]] = ()) -> None:
    """tonnage_estimates.csv (the columns of the reference's tonnage_estimates_combined.csv), tonnage_facilities.csv and tonnage.json;
    numbers by ``repr``, so the files of two runs compare byte for byte.  more_rows: (source, pass, tonnage, tonnage_sd) rows that follow
    the ``Model`` rows (--tonnage-missing)."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, ESTIMATES_FILE), "w") as f:
        f.write("source,pass,tonnage,tonnage_sd\n")
        for p, m, s in zip(est["pass"], est["tonnage"], est["tonnage_sd"]):
            f.write(f"Model,{p},{m!r},{s!r}\n")
        for source, p, m, s in more_rows:
            f.write(f"{source},{p},{m!r},{s!r}\n")
    with open(os.path.join(out_dir, FACILITIES_FILE), "w") as f:
        f.write("facility_index,pass,cages,tonnage,tonnage_sd\n")
        for row in zip(est["facility_index"], est["facility_pass"], est["facility_cages"], est["facility_tonnage"], est["facility_tonnage_sd"]):
            f.write("{},{},{},{!r},{!r}\n".format(*row))
    with open(os.path.join(out_dir, JSON_FILE), "w") as f:
        json.dump({**params, "K": est["K"], "seed": est["seed"], "passes": est["pass"], "tonnage_var": est["tonnage_var"]}, f, indent=1)
        f.write("\n")


def tonnage_from_table(table, out_dir: str, factors_path: str, errors_path: Optional[str] = None, depths_path: Optional[str] = None,
                       K: int = 10000, seed: int = 0, mix: float = 0.5, min_depth: float = DEFAULT_MIN_DEPTH, default_depth: float = DEFAULT_DEPTH,
                       conf_thresh: float = 0.5, eps: float = 10.0, min_cages: int = 5, widths=geocode.IM_WIDTH, heights=geocode.IM_HEIGHT,
                       cpu: bool = False, keep=None, bathymetry: Optional[dict] = None, dedup: Optional[dict] = None,
                       errors: Optional[Dict[Tuple[str, str], Tuple[float, float]]] = None, missing: Optional[dict] = None,
                       near_sites: Optional[str] = None) -> dict:
    """Facilities per image pass (facilities.cluster), their estimates and the three files in `out_dir`.  errors = read_errors' table made
    in this process instead of a file (model_errors.distributions' ``errors``); tonnage.json records it as it records a file's.  bathymetry (bathymetry.settings'
    result, instead of a depths file): the facilities' cage depths come from the depth raster and are written to facility_depths.csv
    beside the three files, in the form `depths_path` takes.  dedup (dedup.dedup_from_table's result, made with the same conf_thresh and
    keep): the survivors of its selection are clustered, and cage_ids_min / cage_ids_max widen the area bounds as the reference's do.
    missing (missing.settings' result; needs dedup): per current pass of its map the facilities of the compare pass that lie outside the
    pass's imagery are added (missing.impute), the imputed table gets one more simulation with the same K and seed, and the rows
    ``Model + Estimate missing`` follow the ``Model`` rows, which stay what they are without it; tonnage_missing_cages.csv and
    tonnage_missing_facilities.csv say why.  near_sites (the known sites' CSV): a further simulation of the facilities cut to the cages
    within 1 km of a site, in tonnage_near_sites.csv."""
    if missing is not None and dedup is None:
        raise ValueError(MISSING_NEEDS_DEDUP)
    if bathymetry is not None and depths_path:
        raise ValueError("tonnage: cage depths come from --bathymetry or from --tonnage-depths, not from both")
    if errors is not None and errors_path:
        raise ValueError("tonnage: model errors come from --model-errors or from --tonnage-errors, not from both")
    factors = read_factors(factors_path)
    errors = read_errors(errors_path) if errors_path else errors
    depths = read_depths(depths_path) if depths_path else None
    if dedup is not None:
        from . import dedup as aqdedup
        fac = aqdedup.cluster(table, dedup, conf_thresh, eps, min_cages, widths, heights, labels_fn=aqfac.dbscan_numpy if cpu else None)
    else:
        fac = aqfac.cluster(table, "pass", conf_thresh, eps, min_cages, widths, heights, labels_fn=aqfac.dbscan_numpy if cpu else None, keep=keep)
    extra = {}
    if bathymetry is not None:
        from . import bathymetry as aqbathy
        cols = aqbathy.depths_of(fac, table, dict(bathymetry, default_depth=float(default_depth), min_depth=float(min_depth)), cpu=cpu)
        depths = {int(fi): float(d) for fi, d in zip(fac["facility_index"], cols["cage_depth"])}
        os.makedirs(out_dir, exist_ok=True)
        defaulted = aqbathy.write_depths_csv(os.path.join(out_dir, aqbathy.DEPTHS_FILE), fac, cols, "pass")
        extra = {"bathymetry": {**aqbathy.describe_settings(bathymetry), "default_depth_facilities": defaulted}}
    est = estimate(fac, None, table, factors, errors, depths, K, seed, mix, min_depth, cpu, default_depth)
    more_rows = []
    if missing is not None or near_sites:
        from . import missing as aqmiss
        again = lambda cut: estimate(cut, None, table, factors, errors, depths, K, seed, mix, min_depth, cpu, default_depth)
        if missing is not None:
            res = aqmiss.missing_estimates(fac, table, missing, again, out_dir, cpu)
            more_rows = [(aqmiss.SOURCE, *row) for row in res["rows"]]
            extra = {**extra, "missing": res["json"]}
            est["missing"] = res
        if near_sites:
            res = aqmiss.near_estimates(fac, table, near_sites, again, out_dir, cpu)
            extra = {**extra, "near_sites": res["json"]}
            est["near_sites"] = res
    device = "cpu"
    if not cpu:
        import torch
        device = torch.cuda.get_device_name(0)
    write_files(out_dir, est, {"device": device, "cpu": bool(cpu), "mix": float(mix), "min_depth": float(min_depth), "default_depth": float(default_depth),
                               "factors": {p: list(v) for p, v in sorted(factors.items())},
                               "errors": [[*k, *v] for k, v in sorted((errors or {}).items())], "depths_file": bool(depths_path),
                               "facilities_conf": float(conf_thresh), "facilities_eps": float(eps), "facilities_min_cages": int(min_cages), **extra,
                               **({"dedup_years": {"selection": dedup["selection"]}} if dedup is not None else {})}, more_rows)
    return est


def describe(est: dict) -> str:
    text = f"{len(est['facility_index'])} facilities, {len(est['pass'])} passes, K = {est['K']}: " + \
        ", ".join(f"{p} {m:.1f} t (sd {s:.1f})" for p, m, s in zip(est["pass"], est["tonnage"], est["tonnage_sd"]))
    if "missing" in est:
        text += "; with missing imagery: " + ", ".join(f"{p} {m:.1f} t (sd {s:.1f}; {est['missing']['json']['passes'][p]['own']} + "
                                                        f"{est['missing']['json']['passes'][p]['added']} facilities)" for p, m, s in est["missing"]["rows"])
    return text


MISSING_NEEDS_DEDUP = ("--tonnage-missing fills a pass's missing imagery from the sweep's blank key and outlines and the facilities' "
                       "cage_ids_min / cage_ids_max: it needs --dedup-years")


def add_options(p: argparse.ArgumentParser) -> None:
    """The options detect.py and this module's command line share."""
    p.add_argument("--tonnage-factors", default=None, metavar="FILE", help="CSV or JSON with pass, s_mean, s_sd, h_mean, h_sd (stocking density kg/m^3, harvests per year)")
    p.add_argument("--tonnage-errors", default=None, metavar="FILE", help="CSV or JSON with pass, farm_type, model_error_mean, model_error_sd (m^2); default zeros")
    p.add_argument("--tonnage-depths", default=None, metavar="FILE", help="CSV or JSON with facility_index, cage_depth (m); default --tonnage-default-depth")
    p.add_argument("--tonnage-default-depth", type=float, default=DEFAULT_DEPTH, metavar="M", help="cage depth of a facility the depth file does not list")
    p.add_argument("--tonnage-min-depth", type=float, default=DEFAULT_MIN_DEPTH, metavar="M", help="smallest cage depth (reference min_cage_threshold)")
    p.add_argument("--tonnage-K", type=int, default=10000, metavar="K", help="simulations of the bootstrap")
    p.add_argument("--tonnage-seed", type=int, default=0, metavar="SEED", help="64-bit seed (the Philox key)")
    p.add_argument("--tonnage-mix", type=float, default=0.5, metavar="P", help="probability of the shallow depth distribution (reference depth_dist_mixture_param)")
    p.add_argument("--tonnage-missing", nargs="?", const="", default=None, metavar="CUR=CMP[,CUR=CMP...]",
                   help="add the rows 'Model + Estimate missing' to tonnage_estimates.csv: per current pass the facilities of the compare pass whose cages "
                        "lie outside the current pass's imagery are added (the reference's compute_complete_period_tonnage_estimates; the box-against-"
                        "coverage test on the GPU); default map: the reference's period_comparison_dict; needs --tonnage and --dedup-years")
    p.add_argument("--tonnage-near-sites", default=None, metavar="CSV",
                   help="also estimate the production of the cages within 1 km of a known site (columns lat, lon; the reference's "
                        "trujillo_comparison) and write tonnage_near_sites.csv; needs --tonnage")


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.tonnage",
                                description="Bootstrap production estimates of the facilities of an existing label directory, without running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv")
    p.add_argument("--out", default=None, metavar="DIR", help="default <labels>/..")
    p.add_argument("--land", default=None, metavar="GEOJSON", help="land polygons: only the detections at sea take part (the --land-filter step)")
    p.add_argument("--image-size", nargs=2, type=int, default=[geocode.IM_WIDTH, geocode.IM_HEIGHT], metavar=("W", "H"),
                   help="pixel size of the images (the border test of the circle areas)")
    p.add_argument("--cpu", action="store_true", help="the numpy restatement instead of the GPU (the same bytes)")
    aqfac.add_options(p)
    add_options(p)
    from . import bathymetry as aqbathy
    aqbathy.add_options(p)
    from . import dedup as aqdedup
    p.add_argument("--dedup-years", nargs=2, default=None, metavar=("BLANK_KEY_CSV", "BLANK_GEOM_GEOJSON"),
                   help="keep one year's cages per tile and pass before clustering (the --dedup-years step), from the sweep's two blank files")
    aqdedup.add_options(p)
    opt = p.parse_args(argv)
    if not opt.tonnage_factors:
        p.error("--tonnage-factors FILE is needed")
    if opt.bathymetry and opt.tonnage_depths:
        p.error("cage depths come from --bathymetry or from --tonnage-depths, not from both")
    miss = None
    if opt.tonnage_missing is not None:
        from . import missing as aqmiss
        if not opt.dedup_years:
            p.error(MISSING_NEEDS_DEDUP)
        try:
            miss = aqmiss.settings(opt.tonnage_missing, opt.dedup_years[0], opt.dedup_years[1], opt.geocode_bboxes)
        except ValueError as e:
            p.error(str(e))
    out = opt.out or os.path.dirname(os.path.abspath(opt.labels.rstrip("/")))
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    keep = None
    if opt.land:
        from . import land as aqland
        segs = aqland.load_land_geojson(opt.land)
        keep = aqland.ocean_rows(table, segs, cpu=opt.cpu)
    bathy = aqbathy.settings(opt.bathymetry, table, keep, opt.bathymetry_statistic) if opt.bathymetry else None
    dd = None
    if opt.dedup_years:
        dd = aqdedup.dedup_from_table(table, opt.dedup_years[0], opt.dedup_years[1], out, opt.dedup_selection, opt.dedup_seed, opt.facilities_conf, keep,
                                      opt.image_size[0], opt.image_size[1], cpu=opt.cpu)
    est = tonnage_from_table(table, out, opt.tonnage_factors, opt.tonnage_errors, opt.tonnage_depths, opt.tonnage_K, opt.tonnage_seed, opt.tonnage_mix,
                             opt.tonnage_min_depth, opt.tonnage_default_depth, opt.facilities_conf, opt.facilities_eps, opt.facilities_min_cages,
                             opt.image_size[0], opt.image_size[1], cpu=opt.cpu, keep=keep, bathymetry=bathy, dedup=dd, missing=miss,
                             near_sites=opt.tonnage_near_sites)
    print(f"{describe(est)} in {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
