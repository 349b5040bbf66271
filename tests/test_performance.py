"""--performance on the host: the stage curves against the reference's procedure done literally (per threshold: filter by confidence, a
brute-force closed-box join both ways with the year and type condition; for the third curve scikit-learn's DBSCAN once per year on all ocean
detections, then the threshold), the strata table against a pandas groupby written as get_bucket_info_table writes it, the sampling
restatement against counts worked out from the stated scheme, the bound's arithmetic, the ABI's refusals without a GPU, and the command
lines.  The inputs and the CPU run are shared with tests/test_gpu_performance.py.

The data: the evaluate fixture's 1,095 detections of 42 images (tests/test_evaluate.py), their confidences scaled per image so that the
images fall into every confidence stratum, three of those images declared land, four left out of the sample, three confidences set to
thresholds, and tests/test_kfold.py's 36 synthetic images without detections."""
import functools
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_evaluate import assert_no_near_ties, detection_table, truth, write_truth_geojson
from test_kfold import kfold_inputs

from aquaculture_amd import evaluate, facilities, kfold, performance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, MIN_CAGES = 50.0, 5
THR100 = np.linspace(0, 1, 100)
R_IMAGES, R_SAMPLE, R_LABELS = 783355, 10518, 4010         # the constants of the reference's upper_bound_calculation.R
PINNED_ALL_ZEROS_50 = [0, 0, 0, 0, 0, 0, 1, 1, 1, 1]         # seed 0, S = 10518, K = 10000, the ten default rates
PINNED_ZERO_SHARE = [0.9056, 0.8164, 0.7355, 0.6576, 0.595, 0.5407, 0.4838, 0.44, 0.3957, 0.3554]


# ---- the shared inputs ----

@functools.lru_cache(maxsize=None)
def inputs():
    """(table, names, rects, sites, land, sample): treat as read-only.  Images 0 .. 41 are the fixture's, in sorted order; their confidences
    are scaled by 0.25 (images 0 .. 4), 0.45 (5 .. 9) and 0.7 (10 .. 15); images 2, 12 and 30 are land; images 3, 7, 20 and 33 and every
    synthetic image on a known site are not in the sample, the synthetic images off the sites all are."""
    names, rects, sites = kfold_inputs()
    table = {k: (v.copy() if k != "stems" else v) for k, v in detection_table().items()}
    stem_row = {s: k for k, s in enumerate(names)}
    det_img = np.asarray([stem_row[evaluate._stem(table["stems"][i])] for i in table["image"]])
    scale = np.ones(len(names))
    scale[0:5], scale[5:10], scale[10:16] = 0.25, 0.45, 0.7
    table["det_conf"] = table["det_conf"] * scale[det_img]
    land = [names[2], names[12] + ".jpeg", names[30]]
    on_land = np.isin(det_img, (2, 12, 30))
    ocean_rows = np.nonzero(~on_land & (det_img >= 16) & ~np.isin(det_img, (20, 33)))[0]
    table["det_conf"][ocean_rows[3]] = THR100[70]           # thresholds that equal a confidence: the >=
    table["det_conf"][ocean_rows[11]] = THR100[85]
    table["det_conf"][np.nonzero(det_img == 30)[0][0]] = 1.0      # the only detection that survives t = 1 is on land
    out_of_sample = {names[k] for k in (3, 7, 20, 33)} | {names[42 + k] for k in range(0, 36, 2)}
    sample = [s for s in names if s not in out_of_sample and s not in {names[2], names[12], names[30]}]
    return table, names, rects, sites, land, sample


@functools.lru_cache(maxsize=None)
def cpu_run(thresholds=100):
    """performance.performance(cpu=True) on inputs() with a small simulation -> (summary, {file: bytes}); computed once and shared."""
    table, names, rects, sites, land, sample = inputs()
    with tempfile.TemporaryDirectory() as d:
        s = performance.performance(table, truth(), d, names=names, sample=sample, land=land, rects=rects, sites=sites, thresholds=thresholds,
                                    eps=EPS, min_cages=MIN_CAGES, rates=(0.01, 0.05, 0.2), K=64, seed=3, cpu=True, device="test")
        return s, {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


class Literal:
    """The reference's procedure: ModelPerformance.py's three sets of sample detections and get_stats_total per threshold."""

    def __init__(self):
        from sklearn.cluster import DBSCAN
        table, names, _, _, land, sample = inputs()
        t = truth()
        cage = np.isin(table["cls"], evaluate.CAGE_CLASSES)
        stem = np.asarray([evaluate._stem(table["stems"][i]) for i in table["image"]], dtype=object)
        on = {evaluate._stem(s) for s in land}
        sampled = np.asarray([s in set(sample) | on for s in stem])          # the land images are appended to the sample
        rows = np.nonzero(cage & sampled)[0]
        self.conf = table["det_conf"][rows]
        self.land = np.asarray([s in on for s in stem[rows]])
        box = np.stack([table[c][rows] for c in evaluate.BOX_COLUMNS], 1)
        lbox = np.stack([t[c] for c in evaluate.BOX_COLUMNS], 1)
        meet = ((box[:, None, 0] <= lbox[None, :, 2]) & (lbox[None, :, 0] <= box[:, None, 2]) & (box[:, None, 1] <= lbox[None, :, 3]) &
                (lbox[None, :, 1] <= box[:, None, 3]))      # the O(n m) join, done once: a threshold only takes rows of it away
        self.meet = meet & (table["year"][rows][:, None] == t["year"][None, :]) & (table["cls"][rows][:, None] == t["cls"][None, :])
        year = table["year"][rows]
        xy = facilities.centroids_3035({c: table[c][rows] for c in evaluate.BOX_COLUMNS})
        self.xy, self.year = xy, year
        self.clustered = np.zeros(rows.shape[0], bool)
        for y in np.unique(year[~self.land]):               # DBSCAN_cluster(cluster_variable='year') on every ocean detection
            idx = np.nonzero(~self.land & (year == y))[0]
            self.clustered[idx[DBSCAN(eps=EPS, min_samples=MIN_CAGES).fit(xy[idx]).labels_ != -1]] = True
        self.domains = [np.ones(rows.shape[0], bool), ~self.land, self.clustered]

    def counts(self, d, t):
        take = self.domains[d] & (self.conf >= t)           # sample_predictions[sample_predictions['det_conf'] >= t]
        return int(take.sum()), int((take & self.meet.any(1)).sum()), self.meet.shape[1], int(self.meet[take].any(0).sum())


@functools.lru_cache(maxsize=None)
def literal():
    return Literal()


# ---- 1. the curves ----

def test_the_data_holds_the_cases_the_curves_can_get_wrong():
    lit = literal()
    assert_no_near_ties({"det": {"xy": lit.xy, "year_id": np.searchsorted(np.unique(lit.year), lit.year)}}, [EPS])
    hit = [lit.meet[dom].any(0) for dom in lit.domains]
    assert (hit[0] & ~hit[1]).any()                         # a label met only by a land detection
    assert (hit[1] & ~hit[2]).any()                         # a label met only by an unclustered detection
    assert (lit.conf == THR100[70]).any() and (lit.conf == THR100[85]).any() and (lit.conf[lit.land] == 1.0).sum() == 1
    assert lit.conf[~lit.land].max() < 1.0                  # ocean: nothing survives t = 1, an empty precision cell
    assert (~lit.meet.any(1) & lit.land).any() and (~lit.meet.any(1) & ~lit.land).any()      # false positives on land and at sea
    assert 0 < lit.clustered.sum() < (~lit.land).sum() < lit.conf.shape[0] < 1095


@pytest.mark.parametrize("N", [100, 2])
def test_curves_equal_the_references_procedure_at_every_threshold(N, tmp_path):
    s, files = cpu_run(N)
    lit = literal()
    path = str(tmp_path / "c.csv")
    with open(path, "wb") as f:
        f.write(files[performance.CURVES_FILE])
    got = performance.read_curves_csv(path)
    thr = np.linspace(0, 1, N)
    assert got["domain"].tolist() == [d for d in performance.DOMAINS for _ in range(N)] and np.array_equal(got["threshold"], np.tile(thr, 3))
    for d in range(3):
        for k, t in enumerate(thr):
            row = d * N + k
            want = lit.counts(d, t)
            assert tuple(int(got[c][row]) for c in ("n_pred", "n_pred_tp", "n_label", "n_label_tp")) == want, (d, t)
            assert got["recall"][row] == want[3] / want[2]
            if want[0]:
                assert got["precision"][row] == want[1] / want[0]
            else:
                assert np.isnan(got["precision"][row])
    ocean_last = files[performance.CURVES_FILE].decode().splitlines()[1 + 2 * N - 1].split(",")
    assert ocean_last[:4] == ["ocean", "1.0", "", "0.0"] and ocean_last[4] == "0"      # the empty cell
    assert got["n_pred"][N - 1] == 1                        # all, t = 1: the land detection of confidence 1 passes the >=
    k70 = 70 if N == 100 else None
    if k70 is not None:
        below = lit.counts(1, np.nextafter(THR100[70], 2.0))
        assert got["n_pred"][N + 70] == below[0] + int((lit.conf[~lit.land] == THR100[70]).sum()) > below[0]


def test_shares_and_reported_rows():
    s, files = cpu_run()
    lit = literal()
    tp = lit.meet.any(1)
    assert s["fp_share_raw"] == 100 - 100 * int(tp.sum()) / tp.shape[0] and 0 < s["fp_share_raw"] < 100
    assert s["land_fp_dropped"] == 100 - 100 * int((~tp & ~lit.land).sum()) / int((~tp).sum()) and 0 < s["land_fp_dropped"] < 100
    assert s["land_images"] is True and s["n_land_images"] == 3 and s["n_detections"] == tp.shape[0] and s["n_labels"] == 991
    assert json.loads(files[performance.JSON_FILE]) == s and b"NaN" not in files[performance.JSON_FILE]
    rows = s["reported_rows"]
    assert [(r["rule"], r["domain"], r["min_threshold"]) for r in rows] == [
        ("lowest precision", "all", 0.0), ("lowest precision", "all", 0.5), ("lowest precision", "all", 0.8), ("lowest precision", "ocean", 0.8),
        ("lowest precision", "ocean + clustered", 0.8), ("first row", "ocean", 0.75)]
    for r in rows[:5]:
        d = performance.DOMAINS.index(r["domain"])
        cand = [(lit.counts(d, t), t) for t in THR100 if t >= r["min_threshold"]]
        prec = [(c[1] / c[0] if c[0] else math.inf, t) for c, t in cand]
        assert (r["row"]["precision"], r["row"]["threshold"]) == min(prec)      # NaN last, a tie to the smaller threshold
    assert rows[5]["row"]["threshold"] == THR100[75] and rows[5]["row"]["n_pred"] == lit.counts(1, THR100[75])[0]
    # a tie and an empty cell, by hand
    t = {"domain": np.asarray(["all"] * 4, dtype=object), "threshold": np.array([0.0, 0.5, 0.8, 1.0]), "precision": np.array([0.5, 0.4, 0.4, np.nan]),
         "recall": np.ones(4), **{c: np.ones(4, np.int64) for c in ("n_pred", "n_pred_tp", "n_label", "n_label_tp")}}
    got = performance.reported_rows(t)
    assert [g["row"]["threshold"] for g in got[:3]] == [0.5, 0.5, 0.8] and got[3]["row"] is None and got[5]["row"] is None
    t["precision"][:] = np.nan
    assert performance.reported_rows(t)[0]["row"]["threshold"] == 0.0 and performance.reported_rows(t)[0]["row"]["precision"] is None


def test_without_land_images_no_image_leaves_the_ocean(tmp_path):
    table, names, rects, sites, land, sample = inputs()
    s = performance.performance(table, truth(), str(tmp_path), names=names, sample=sample, rects=rects, sites=sites, thresholds=5, K=2,
                                rates=(0.5,), cpu=True)
    assert s["land_images"] is False and s["n_land_images"] == 0 and s["land_fp_dropped"] == 0.0 and s["device"] == "cpu"
    got = performance.read_curves_csv(str(tmp_path / performance.CURVES_FILE))
    assert np.array_equal(got["n_pred"][:5], got["n_pred"][5:10]) and [r["bucket"] for r in s["strata"]] == list(kfold.STRATA)


# ---- 2. the strata table ----

def test_strata_table_is_the_references_groupby(tmp_path):
    import pandas as pd
    table, names, rects, sites, land, sample = inputs()
    s, files = cpu_run()
    t = truth()
    on = {evaluate._stem(x) for x in land}
    det_stem = pd.Series([evaluate._stem(table["stems"][i]) for i in table["image"]])
    lab_stem = pd.Series([evaluate._stem(x) for x in t["image"]])
    images = pd.DataFrame({"image": names})
    images["only_land"] = images["image"].isin(on)
    images["in_sample"] = images["image"].isin(set(sample) | on)
    images["num_detections"] = images["image"].map(det_stem.value_counts()).fillna(0).astype(int)
    images["det_conf"] = images["image"].map(pd.Series(table["det_conf"]).groupby(det_stem.values).max())
    images["num_labels_sample"] = images["image"].map(lab_stem.value_counts()).fillna(0)
    images.loc[~images["in_sample"], "num_labels_sample"] = np.nan          # set_image_stats
    known = kfold.in_known_area(rects, sites)
    cut = pd.cut(images["det_conf"], bins=[0, 0.3, 0.5, 0.8, 1]).astype(object)
    images["bucket"] = [kfold.LAND if l else (kfold.NO_DET_IN if k else kfold.NO_DET_OUT) if pd.isna(c) else str(c)
                        for c, l, k in zip(cut, images["only_land"], known)]
    num_in_sample = lambda x: len(x[images.loc[x.index, "in_sample"]])
    sum_in_sample = lambda x: x[images.loc[x.index, "in_sample"]].sum()
    info = images.groupby("bucket").agg(num_detections_bucket=("num_detections", "sum"), num_detections_sample=("num_detections", sum_in_sample),
                                        num_images_bucket=("image", "size"), num_images_sample=("image", num_in_sample),
                                        num_labels_sample=("num_labels_sample", "sum"))
    info["estimated_num_labels_bucket"] = (info["num_labels_sample"] / info["num_images_sample"]) * info["num_images_bucket"]
    path = str(tmp_path / "s.csv")
    with open(path, "wb") as f:
        f.write(files[performance.STRATA_FILE])
    got = performance.read_strata_csv(path)
    assert [r["bucket"] for r in got] == list(kfold.STRATA) + [kfold.LAND] and got == s["strata"]
    assert files[performance.STRATA_FILE].decode().splitlines()[0] == ",".join(performance.STRATA_COLUMNS)
    for r in got:
        w = info.loc[r["bucket"]]
        for c in performance.STRATA_COLUMNS[1:6]:
            assert r[c] == int(w[c]), (r["bucket"], c)
        if w["num_images_sample"] == 0:
            assert r["estimated_num_labels_bucket"] is None and np.isnan(w["estimated_num_labels_bucket"])
        else:
            assert r["estimated_num_labels_bucket"] == float(w["estimated_num_labels_bucket"]), r["bucket"]
    by = {r["bucket"]: r for r in got}
    full, part, none = by["(0.0, 0.3]"], by["(0.8, 1.0]"], by[kfold.NO_DET_IN]
    assert 0 < part["num_images_sample"] < part["num_images_bucket"] and by[kfold.NO_DET_OUT]["num_images_sample"] == by[kfold.NO_DET_OUT]["num_images_bucket"] == 18
    assert 0 < full["num_images_bucket"] and all(by[b]["num_images_bucket"] > 0 for b in kfold.STRATA)
    assert none["num_images_sample"] == 0 and none["num_images_bucket"] == 18 and f"{kfold.NO_DET_IN}\",18,0,0,0,0,\n" in files[performance.STRATA_FILE].decode()
    assert by[kfold.LAND]["num_images_sample"] == by[kfold.LAND]["num_images_bucket"] == 3
    # labels outside the sample do not count: images 3, 7, 20 and 33 hold labels
    outside = sum(int((lab_stem == names[k]).sum()) for k in (3, 7, 20, 33))
    assert outside > 0 and sum(r["num_labels_sample"] for r in got) == 991 - outside


# ---- 3. the sampling and the bound ----

def test_sampling_restatement_gives_the_counts_of_the_stated_scheme():
    rates = (0.0, 1.0, 0.5, 2.0 ** -53)
    c = performance.counts_numpy(5, 0, 3, 129, rates)
    assert c.dtype == np.int32 and c.tolist() == [[0, 129, 69, 0], [0, 129, 76, 0], [0, 129, 66, 0]]
    # one draw spelled out: j = 128 of simulation 2 is the even half of call 64
    from aquaculture_amd.tonnage import philox4x32, uniform_from_words
    w = philox4x32(2, 64, 16, 0, 5, 0)
    u_last = float(uniform_from_words(w[0], w[1]))
    assert performance.counts_numpy(5, 2, 1, 129, (0.5,))[0, 0] - performance.counts_numpy(5, 2, 1, 128, (0.5,))[0, 0] == int(u_last < 0.5)
    w = philox4x32(2, 63, 16, 0, 5, 0)                      # and j = 127 the odd half of call 63
    assert performance.counts_numpy(5, 2, 1, 128, (0.5,))[0, 0] - performance.counts_numpy(5, 2, 1, 127, (0.5,))[0, 0] == int(float(uniform_from_words(w[2], w[3])) < 0.5)
    # monotone in the rate for every simulation; k0-chunks equal one call; a high key word and a high counter word
    rates = np.array([0.0, 0.01, 0.3, 0.3, 0.62, 0.9, 1.0])
    for seed, k0 in ((0, 0), ((1 << 63) + 5, (1 << 32) - 9)):
        one = performance.counts_numpy(seed, k0, 9, 257, rates)
        assert (np.diff(one, axis=1) >= 0).all() and (one[:, 2] == one[:, 3]).all() and (one[:, 0] == 0).all() and (one[:, -1] == 257).all()
        parts = np.concatenate([performance.counts_numpy(seed, k0, 4, 257, rates), performance.counts_numpy(seed, k0 + 4, 5, 257, rates)])
        assert np.array_equal(one, parts) and np.array_equal(one, performance.counts_numpy(seed, k0, 9, 257, rates, block=100))
    assert not np.array_equal(performance.counts_numpy(0, 0, 9, 257, rates), performance.counts_numpy(1 << 32, 0, 9, 257, rates))
    assert performance.counts_numpy(0, 0, 0, 5, (0.5,)).shape == (0, 1)
    for bad in (dict(S=0), dict(S=1 << 31), dict(K=-1), dict(k0=-1), dict(k0=(1 << 32) - 1, K=2), dict(rates=(1.5,)), dict(rates=(float("nan"),)),
                dict(rates=()), dict(rates=(0.1,) * 17)):
        kw = {**dict(seed=0, k0=0, K=1, S=10, rates=(0.5,)), **bad}
        with pytest.raises(ValueError):
            performance.counts_numpy(**kw)
    assert performance.chunk_sizes(10000, 10518) == [10000] and performance.chunk_sizes(5, 1 << 30) == [4, 1] and performance.chunk_sizes(3, (1 << 31) - 1) == [2, 1]


def test_simulation_at_the_references_sample_size():
    S, K, rates = R_SAMPLE, 1000, (4e-5, 1e-4)
    sim = performance.simulate(K, S, rates, 0, cpu=True)
    assert tuple(sim["all_zeros_50"]) == (0, 1)
    for share, r in zip(sim["zero_share"], rates):
        p = (1 - r) ** S
        assert abs(share - p) <= 5 * math.sqrt(p * (1 - p) / K), (share, p)
    assert sim["zero_share"] == [z / K for z in sim["zeros"]]
    with pytest.raises(ValueError, match="at least 2"):
        performance.simulate(1, 10, (0.5,), cpu=True)


def test_the_bounds_arithmetic():
    b = performance.population_bound(performance.DEFAULT_RATES, [0] * 6 + [1] * 4, PINNED_ZERO_SHARE, R_IMAGES, R_SAMPLE, R_LABELS)
    assert b["final_rate"] == performance.DEFAULT_RATES[6] == 7 * 1e-5 and math.isclose(b["final_rate"], 7e-05, rel_tol=1e-15)
    assert (b["images_with_cages"], b["stratum_estimate"], b["upper_bound"]) == (55, 275, 4285)
    assert (b["images_stratum"], b["sample_stratum"], b["labels_other_strata"], b["cages_per_image"], b["K"], b["seed"]) == (R_IMAGES, R_SAMPLE, R_LABELS, 5.0, 10000, 0)
    assert performance.population_bound((7e-05,), [1], [0.4], R_IMAGES, R_SAMPLE, R_LABELS)["upper_bound"] == 4285
    none = performance.population_bound(performance.DEFAULT_RATES, [0] * 10, PINNED_ZERO_SHARE, R_IMAGES, R_SAMPLE, R_LABELS)
    assert none["final_rate"] is None and none["upper_bound"] is None and none["images_with_cages"] is None and none["stratum_estimate"] is None
    assert performance.population_bound((0.3, 0.1, 0.2), [2, 0, 1], [0, 0, 0], 10, 5, 0)["final_rate"] == 0.2       # the smallest rate, not the first
    assert performance.population_bound((0.25,), [1], [0], 10, 5, 1)["images_with_cages"] == 2                      # round half to even, as R
    rows = [{"bucket": b_, "num_images_bucket": 10, "num_images_sample": 4, "num_labels_sample": 7} for b_ in kfold.STRATA + (kfold.LAND,)]
    rows[5]["num_images_sample"] = 0
    assert performance.bound_from_strata(rows, (0.5,), K=4, cpu=True) == {"skipped": f"no sampled image in the stratum '{kfold.NO_DET_OUT}'"}
    rows[5].update(num_images_sample=4, num_images_bucket=100)
    got = performance.bound_from_strata(rows, (1.0,), K=4, seed=1, cages_per_image=2.0, cpu=True)      # every draw a success: final_rate 1
    assert got["labels_other_strata"] == 35 and got["images_stratum"] == 100 and got["sample_stratum"] == 4 and got["all_zeros_50"] == [4]
    assert got["upper_bound"] == 100 * 2.0 + 35
    s, _ = cpu_run()
    by = {r["bucket"]: r for r in s["strata"]}
    pb = s["population_bound"]
    assert pb["sample_stratum"] == 18 and pb["images_stratum"] == 18 and pb["K"] == 64 and pb["seed"] == 3 and pb["rates"] == [0.01, 0.05, 0.2]
    assert pb["labels_other_strata"] == sum(by[b_]["num_labels_sample"] for b_ in kfold.STRATA[:5])
    assert pb["all_zeros_50"] == np.sort(performance.counts_numpy(3, 0, 64, 18, (0.01, 0.05, 0.2)), 0)[31].tolist()


# ---- the ABI ----

def test_symbol_is_declared_exported_bound_and_refuses_without_a_gpu(lib):
    import ctypes as C
    from aquaculture_amd import build, engine
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    name = "aq_bernoulli_counts_i32"
    assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name)
    fn = getattr(lib, name)
    assert fn.argtypes == [C.c_ulonglong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int and callable(engine.bernoulli_counts) and engine.BERNOULLI_MAX_RATES == performance.MAX_RATES == 16
    assert ("population.hip", ["-ffp-contract=off"]) in build.SOURCES
    csrc = os.path.join(ROOT, "aquaculture_amd", "csrc")
    assert '#include "philox.h"' in open(os.path.join(csrc, "tonnage.hip")).read() and '#include "philox.h"' in open(os.path.join(csrc, "population.hip")).read()
    assert sum("PHILOX_M0 =" in open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".h"))) == 1     # written once
    rates = (C.c_double * 16)(*([0.5] * 16))
    ok = dict(seed=0, k0=0, K=1, S=10, rates=rates, R=3)
    call = lambda **kw: (lambda a: fn(a["seed"], a["k0"], a["K"], a["S"], None, a["rates"], a["R"], None, None))({**ok, **kw})
    for kw in (dict(R=0), dict(R=17), dict(R=-1), dict(S=0), dict(S=1 << 31), dict(S=-5), dict(K=-1), dict(k0=-1), dict(k0=(1 << 32) - 1, K=2),
               dict(k0=1 << 32, K=1), dict(k0=0, K=(1 << 32) + 1), dict(rates=(C.c_double * 3)(0.5, float("nan"), 0.5)), dict(rates=(C.c_double * 3)(0.5, 0.5, 1.5)),
               dict(rates=(C.c_double * 3)(-1e-300, 0.5, 0.5)), dict(rates=None)):
        assert call(**kw) != 0, kw
        assert lib.aq_last_error().startswith(b"population:"), kw
    assert call() != 0 and b"null pointer" in lib.aq_last_error()          # everything in range: the arrays are looked at last, before any launch
    assert call(K=0) == 0 and call(K=0, k0=1 << 32) == 0                   # nothing to do
    assert call(K=0, rates=(C.c_double * 3)(0.0, 1.0, 0.5)) == 0


# ---- the command lines ----

def test_options_and_refusals(tmp_path):
    from aquaculture_amd import detect
    base = ["--evaluate", "truth.geojson", "--geocode-bboxes", "wb.csv"]
    opt = detect.parse_opt(base)
    assert opt.performance is None and detect.parse_opt([]).performance is None
    opt = detect.parse_opt(base + ["--performance"])
    assert (opt.performance, opt.performance_sample, opt.performance_thresholds, opt.performance_eps, opt.performance_min_cages, opt.performance_rates,
            opt.performance_K, opt.performance_seed, opt.performance_cages_per_image) == ("", None, 100, 50.0, 5, None, 10000, 0, 5.0)
    opt = detect.parse_opt(base + ["--performance", "out", "--performance-sample", "cf.csv", "--performance-thresholds", "11", "--performance-rates", "0.1,0.2",
                                   "--performance-K", "50", "--performance-seed", "9", "--performance-cages-per-image", "4.5", "--performance-eps", "30",
                                   "--performance-min-cages", "3"])
    assert (opt.performance, opt.performance_sample, opt.performance_thresholds, opt.performance_rates, opt.performance_K, opt.performance_seed,
            opt.performance_cages_per_image, opt.performance_eps, opt.performance_min_cages) == ("out", "cf.csv", 11, "0.1,0.2", 50, 9, 4.5, 30.0, 3)
    for bad in (["--performance"], ["--performance", "--evaluate", "t.geojson"], ["--performance", "--geocode-bboxes", "wb.csv"],
                base + ["--performance", "--performance-thresholds", "1"], base + ["--performance", "--performance-K", "1"],
                base + ["--performance", "--performance-rates", "0.5,1.5"], base + ["--performance", "--performance-rates", "0:0.17:0.01"],
                base + ["--performance", "--performance-eps", "0"], base + ["--performance", "--tile-scenes"]):
        with pytest.raises(SystemExit):
            detect.parse_opt(bad)
    assert detect.parse_opt(base + ["--performance", "--tile-scenes", "--evaluate-kfold-images", "i.txt"]).performance == ""
    with pytest.raises(ValueError, match="--evaluate TRUTH_GEOJSON"):
        detect.run("w.pt", "src", performance="")
    with pytest.raises(ValueError, match="--geocode-bboxes"):
        detect.run("w.pt", "src", performance="", evaluate="t.geojson")
    with pytest.raises(ValueError, match="--evaluate TRUTH_GEOJSON"):
        detect.run("w.pt", "src", performance="", geocode_bboxes="wb.csv")
    with pytest.raises(ValueError, match="--evaluate-kfold-images FILE"):
        detect.run("w.pt", "src", performance="", evaluate="t.geojson", geocode_bboxes="wb.csv", tile_scenes=1024)
    with pytest.raises(ValueError, match="at least 2"):
        detect.run("w.pt", "src", performance="", evaluate="t.geojson", geocode_bboxes="wb.csv", performance_K=1)
    assert "performance" not in detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True)
    assert performance.check_options(100, 50, 5, "1e-5:1.05e-4:1e-5", 10).shape == (10,) and performance.check_options(2, 1, 1, None, 2).tolist() == list(performance.DEFAULT_RATES)
    with pytest.raises(SystemExit):
        performance.main(["--labels", "l", "--geocode-bboxes", "wb.csv"])                  # --truth is required
    with pytest.raises(SystemExit):
        performance.main(["--labels", "l", "--truth", "t.geojson"])                        # and so is --geocode-bboxes
    with pytest.raises(SystemExit):
        performance.main(["--labels", "l", "--geocode-bboxes", "wb.csv", "--truth", "t.geojson", "--performance-K", "1"])
    (tmp_path / "cf.csv").write_text("id,image,who\n1,a.jpeg,x\n\n2,dir/b.png,y\n")
    (tmp_path / "cf.txt").write_text("a.jpeg\n\nb\n")
    assert performance.read_sample(str(tmp_path / "cf.csv")) == ["a.jpeg", "dir/b.png"] and performance.read_sample(str(tmp_path / "cf.txt")) == ["a.jpeg", "b"]


def test_module_command_line_writes_the_three_files_and_evaluate_alone_none_of_them(tmp_path):
    from test_tonnage import synthetic_run
    from aquaculture_amd import geocode
    labels, bboxes = synthetic_run(tmp_path)
    table = geocode.geocode_label_dir(labels, bboxes)
    feats = []
    for k in range(0, table["cls"].shape[0], 2):            # every other detection has a label in its place
        x0, y0, x1, y1 = (float(table[c][k]) for c in evaluate.BOX_COLUMNS)
        kind = "circle_cage" if table["cls"][k] == facilities.CLS_OF["circle_farm"] else "square_cage"
        feats.append({"type": "Feature", "properties": {"image": str(table["stems"][table["image"][k]]) + ".jpeg", "type": kind, "year": int(table["year"][k])},
                      "geometry": {"type": "Polygon", "coordinates": [[[x1, y0], [x1, y1], [x0, y1], [x0, y0], [x1, y0]]]}})
    truth_path = tmp_path / "truth.geojson"
    truth_path.write_text(json.dumps({"type": "FeatureCollection", "crs": {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::3857"}}, "features": feats}))
    plain = tmp_path / "plain"
    assert evaluate.main(["--labels", labels, "--geocode-bboxes", bboxes, "--truth", str(truth_path), "--cpu", "--evaluate-out", str(plain),
                          "--evaluate-conf", "0.5", "--evaluate-eps", "50", "--evaluate-min-cages", "3"]) == 0
    assert sorted(os.listdir(plain)) == [evaluate.CSV_FILE, evaluate.JSON_FILE]           # without the flag: none of the three
    (tmp_path / "cf.csv").write_text("image\nORTHOIMAGERY.ORTHOPHOTOS2015_3_0_0.jpeg\nORTHOIMAGERY.ORTHOPHOTOS2015_3_1024_0\n")
    out = tmp_path / "perf"
    r = subprocess.run([sys.executable, "-m", "aquaculture_amd.performance", "--labels", labels, "--geocode-bboxes", bboxes, "--truth", str(truth_path), "--cpu",
                        "--out", str(out), "--performance-sample", str(tmp_path / "cf.csv"), "--performance-thresholds", "5", "--performance-eps", "30",
                        "--performance-min-cages", "3", "--performance-rates", "0.1,0.5", "--performance-K", "16", "--performance-seed", "2"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == sorted([performance.CURVES_FILE, performance.STRATA_FILE, performance.JSON_FILE]) and "population bound" in r.stdout
    s = json.load(open(out / performance.JSON_FILE))
    assert s["device"] == "cpu" and s["land_images"] is False and s["n_images"] == 3 and s["n_sampled_images"] == 2 and s["n_labels"] == len(feats)
    assert s["parameters"] == {"thresholds": 5, "eps": 30.0, "min_cages": 3, "rates": [0.1, 0.5], "K": 16, "seed": 2, "cages_per_image": 5.0, "known_sites": 0}
    curves = performance.read_curves_csv(str(out / performance.CURVES_FILE))
    assert curves["n_pred"].shape == (15,) and curves["n_pred"][0] == 14 and (curves["n_label"] == len(feats)).all()      # the 2012 image is not in the sample
    assert s["population_bound"] == {"skipped": f"no sampled image in the stratum '{kfold.NO_DET_OUT}'"}
    assert [r_["bucket"] for r_ in performance.read_strata_csv(str(out / performance.STRATA_FILE))] == list(kfold.STRATA)
