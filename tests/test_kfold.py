"""--evaluate-kfold on the host: the splits against scikit-learn's train_test_split and StratifiedKFold index for index, the strata against
pandas.cut, the numpy restatements of the two subset kernels against the single-set restatements of tests/test_evaluate.py run on every
subset alone, and the whole cross-validation against the reference's procedure done literally per fold (scikit-learn's DBSCAN per grid
point and year on the fold's detections, brute-force joins with the fold's labels) on the evaluate fixture plus synthetic images without
detections; the options, the files and the ABI surface.  The inputs are shared with tests/test_gpu_kfold.py."""
import functools
import json
import os
import warnings

import numpy as np
import pytest

from test_evaluate import SMALL_GRID, Oracle, assert_no_near_ties, detection_table, truth, write_truth_geojson
from test_facilities import CASES

from aquaculture_amd import evaluate, kfold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SITES = os.path.join(ROOT, "tests", "golden", "g14_known_sites.csv")
BBOXES = os.path.join(ROOT, "tests", "golden", "g14_wanted_bboxes.csv")
NEG_INF = float("-inf")


# ---- the splits ----

def strata_codes(n, seed, classes=6):
    return np.random.default_rng(seed).integers(0, classes, n)


@pytest.mark.parametrize("n", [40, 57, 286, 1000])
def test_holdout_and_folds_are_scikit_learns_index_for_index(n):
    from sklearn.model_selection import StratifiedKFold, train_test_split
    y = strata_codes(n, n)
    for seed in (0, 1, 7):
        train, test = kfold.holdout_split(n, 0.1, seed)
        want_train, want_test, y_train, _ = train_test_split(np.arange(n), y, test_size=0.1, random_state=seed)
        assert np.array_equal(train, want_train) and np.array_equal(test, want_test)
        for N in (2, 5, 10):
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    want = list(StratifiedKFold(n_splits=N, shuffle=True, random_state=seed).split(train, y_train))
            except ValueError:                              # n = 40, N = 10: no class has 10 members; scikit-learn refuses, and so does this
                assert n == 40 and N == 10
                with pytest.raises(ValueError, match="largest stratum"):
                    kfold.stratified_folds(y[train], N, seed)
                continue
            fold = kfold.stratified_folds(y[train], N, seed)
            assert len(want) == N
            for k, (tr, te) in enumerate(want):
                assert np.array_equal(np.nonzero(fold != k)[0], tr) and np.array_equal(np.nonzero(fold == k)[0], te), (n, seed, N, k)
            split = kfold.split_images(y, N, seed, 0.1)
            assert np.array_equal(np.nonzero(split < 0)[0], np.sort(want_test)) and np.array_equal(split[train], fold)


def test_small_classes_a_single_class_other_fractions_and_the_refusals():
    from sklearn.model_selection import StratifiedKFold, train_test_split
    y = np.array([3] * 30 + [1] * 2 + [9] * 7 + [4])          # classes of 2 and 1 members: scikit-learn warns and still splits
    y = y[np.random.default_rng(2).permutation(40)]
    for ys in (y, np.zeros(40, np.int64)):
        for N in (2, 5, 10):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = list(StratifiedKFold(n_splits=N, shuffle=True, random_state=1).split(ys, ys))
            fold = kfold.stratified_folds(ys, N, 1)
            for k, (tr, te) in enumerate(want):
                assert np.array_equal(np.nonzero(fold == k)[0], te) and np.array_equal(np.nonzero(fold != k)[0], tr)
    for n, frac in ((30, 0.1), (57, 0.25), (10, 0.33), (1000, 0.07)):      # 0.1 * 30 is a little above 3: four rows are set aside
        train, test = kfold.holdout_split(n, frac, 3)
        a, b = train_test_split(np.arange(n), test_size=frac, random_state=3)
        assert np.array_equal(train, a) and np.array_equal(test, b), (n, frac)
    train, test = kfold.holdout_split(9, 0, 1)
    assert train.tolist() == list(range(9)) and test.shape == (0,)
    with pytest.raises(ValueError, match="at least 2"):
        kfold.stratified_folds(y, 1, 1)
    with pytest.raises(ValueError, match="largest stratum"):
        kfold.stratified_folds(y, 31, 1)
    with pytest.raises(ValueError):
        StratifiedKFold(n_splits=31, shuffle=True, random_state=1).split(y, y).__next__()
    with pytest.raises(ValueError, match="32 bits"):
        kfold.split_images(np.zeros(400, np.int64), 16, 1, 0.1)
    with pytest.raises(ValueError, match="at least 2"):
        kfold.split_images(np.zeros(400, np.int64), 1, 1, 0.1)
    assert kfold.split_images(np.zeros(400, np.int64), 15, 1, 0.1).max() == 14
    with pytest.raises(ValueError, match="fraction"):
        kfold.holdout_split(10, 1.0, 1)


def test_subset_words():
    w = kfold.subset_words(np.array([-1, 0, 2, 14]), 15)
    assert w.dtype == np.uint32 and w[0] == 1 << 30 and w[3] == (1 << 31) | (1 << 29) | (0x7FFF & ~(1 << 14))
    w = kfold.subset_words(np.array([-1, 0, 1, 2]), 3)
    assert w.tolist() == [1 << 6, 0b10001110, 0b10010101, 0b10100011]


# ---- the strata ----

def test_buckets_are_pandas_cut_at_every_edge():
    import pandas as pd
    edges = [0.3, 0.5, 0.8, 1.0]
    conf = np.array([v for e in edges for v in (np.nextafter(e, 0.0), e, np.nextafter(e, 2.0))] + [0.0, np.nextafter(0.0, 1.0), 0.65, np.nan, 1.5])
    cut = pd.cut(pd.Series(conf), bins=[0, 0.3, 0.5, 0.8, 1])
    want = [kfold.NO_DET_OUT if pd.isna(v) else str(v) for v in cut]
    got = [kfold.STRATA[k] for k in kfold.buckets(conf, np.zeros(conf.shape[0], bool))]
    assert got == want and len(set(got)) == 5
    assert [str(c) for c in cut.cat.categories] == list(kfold.INTERVALS)
    known = np.arange(conf.shape[0]) % 2 == 0
    got = [kfold.STRATA[k] for k in kfold.buckets(conf, known)]
    assert got == [(kfold.NO_DET_IN if kn else kfold.NO_DET_OUT) if w == kfold.NO_DET_OUT else w for w, kn in zip(want, known)]


def test_a_site_box_that_touches_counts_one_ulp_away_does_not():
    site = np.array([[500000.0, 5300000.0]])
    x1, y1 = site[0, 0] + 1000.0, site[0, 1] + 1000.0
    up = lambda v: np.nextafter(v, np.inf)
    rects = np.array([[x1, y1 - 300.0, x1 + 200.0, y1 - 100.0],               # shares the box's east edge
                      [up(x1), y1 - 300.0, x1 + 200.0, y1 - 100.0],           # one ulp east of it
                      [x1, y1, x1 + 200.0, y1 + 200.0],                       # touches at the north-east corner
                      [up(x1), y1, x1 + 200.0, y1 + 200.0], [x1, up(y1), x1 + 200.0, y1 + 200.0],
                      [site[0, 0] - 1200.0, site[0, 1] - 1200.0, site[0, 0] - 1000.0, site[0, 1] - 1000.0],      # the south-west corner
                      [site[0, 0] - 1200.0, site[0, 1] - 1200.0, np.nextafter(site[0, 0] - 1000.0, 0.0), site[0, 1] - 1000.0],
                      [site[0, 0] - 5.0, site[0, 1] - 5.0, site[0, 0] + 5.0, site[0, 1] + 5.0],                  # inside
                      [site[0, 0] - 5000.0, site[0, 1] - 5000.0, site[0, 0] + 5000.0, site[0, 1] + 5000.0]])     # around
    assert kfold.in_known_area(rects, site).tolist() == [True, False, True, False, False, True, False, True, True]
    assert not kfold.in_known_area(rects, None).any() and not kfold.in_known_area(rects, np.zeros((0, 2))).any()
    try:
        from shapely.geometry import box
    except ImportError:
        return
    b = box(site[0, 0] - 1000, site[0, 1] - 1000, site[0, 0] + 1000, site[0, 1] + 1000)
    assert [box(*r).intersects(b) for r in rects] == kfold.in_known_area(rects, site).tolist()


def test_known_sites_file():
    from aquaculture_amd import geocode
    sites = kfold.load_known_sites(SITES)
    rows = [l.split(",") for l in open(SITES).read().splitlines()[1:]]
    assert sites.shape == (len(rows), 2) and len(rows) == 20 and os.path.getsize(SITES) < 4096
    x, y = geocode.lonlat_to_mercator(np.float64(rows[3][2]), np.float64(rows[3][1]))
    assert sites[3].tolist() == [float(x), float(y)]


# ---- the fixture with synthetic images ----

N_SYNTH = 36


@functools.lru_cache(maxsize=None)
def kfold_inputs():
    """The evaluate fixture's 42 images (rectangles from their names and the two scenes' boxes) and 36 synthetic images without detections or
    labels, every other one on a known site, the others 300 km south of any -> (names, rects, sites); treat as read-only."""
    sites = kfold.load_known_sites(SITES)
    names = sorted({evaluate._stem(s) for s in truth()["image"]})
    rect_of = kfold.tile_rects(BBOXES)
    rects = [rect_of(s) for s in names]
    for k in range(N_SYNTH):
        x, y = sites[k % sites.shape[0]]
        y -= 0.0 if k % 2 == 0 else 3.0e5
        names.append(f"ORTHOIMAGERY.ORTHOPHOTOS{2003 + k % 3}_9{k:03d}_0_0")
        rects.append((x - 100.0, y - 100.0, x + 100.0, y + 100.0))
    return names, np.asarray(rects, np.float64), sites


@functools.lru_cache(maxsize=None)
def fixture_images():
    """(data, images, names): evaluate.inputs of the fixture and kfold.image_table over kfold_inputs(); treat as read-only."""
    names, rects, sites = kfold_inputs()
    table, t = detection_table(), truth()
    data = evaluate.inputs(table, t)
    det_image = [str(table["stems"][i]) for i in table["image"][data["det"]["rows"]]]
    images = kfold.image_table(names, det_image, data["det"]["conf"], [str(s) for s in t["image"][data["lab"]["rows"]]], rects, sites)
    return data, images, names


def test_image_table_of_the_fixture_and_the_synthetic_images():
    data, images, names = fixture_images()
    assert len(names) == 42 + N_SYNTH and images["n_detections"].sum() == 1095 and images["n_labels"].sum() == 991
    assert (images["n_detections"][42:] == 0).all() and np.isnan(images["det_conf"][42:]).all() and images["in_known_area"][:42].all()
    table = detection_table()
    for k in (0, 7, 41):
        mine = np.asarray([table["stems"][i] == names[k] for i in table["image"]])
        assert images["n_detections"][k] == mine.sum() and images["det_conf"][k] == table["det_conf"][mine].max()
    assert images["in_known_area"][42:].tolist() == [k % 2 == 0 for k in range(N_SYNTH)]
    counts = {s["bucket"]: s["images"] for s in kfold.strata_table(images)}
    assert counts == {"(0.0, 0.3]": 0, "(0.3, 0.5]": 0, "(0.5, 0.8]": 1, "(0.8, 1.0]": 41, kfold.NO_DET_IN: 18, kfold.NO_DET_OUT: 18}
    assert images["year"][0] == 2003 and (images["det_row"] >= 0).all() and (images["lab_row"] >= 0).all()
    part = kfold.image_table(names[5:], ["x/" + names[5] + ".jpeg", names[0]], [0.5, 0.9], [names[6] + ".jpeg"])
    assert part["det_row"].tolist() == [0, -1] and part["lab_row"].tolist() == [1] and part["det_conf"][0] == 0.5 and not part["in_known_area"].any()
    with pytest.raises(ValueError, match="twice"):
        kfold.image_table([names[0], names[0] + ".jpeg"], [], [], [])
    with pytest.raises(ValueError, match="rectangles"):
        kfold.image_table(names, [], [], [], None, kfold_inputs()[2])


# ---- the restatements of the two kernels ----

def subset_masks(n, S, seed):
    """uint32 [n]: random words of S bits; subset 0 is empty, the last one full (S > 1), points 0 and 1 are in no subset (but the full one)."""
    r = np.random.default_rng(seed)
    m = r.integers(0, 1 << S, n, dtype=np.uint64).astype(np.uint32)
    if S > 1:
        m &= ~np.uint32(1)
        m[:2] = 0
        m |= np.uint32(1 << (S - 1))
        m[:2] &= ~np.uint32(1 << (S - 1)) if S > 2 else np.uint32(0xFFFFFFFF)
    return m


def member_by_subset(xy, group, conf, mask, eps, K, S):
    """evaluate.member_conf_numpy on the points of every subset alone, scattered back."""
    out = np.full((S, xy.shape[0], K), NEG_INF)
    for s in range(S):
        idx = np.nonzero((mask >> np.uint32(s)) & np.uint32(1))[0]
        if idx.shape[0]:
            out[s, idx] = evaluate.member_conf_numpy(xy[idx], group[idx], conf[idx], eps, K)
    return out


def match_by_subset(qbox, qgroup, qmask, kbox, kgroup, kmask, S, payload=None):
    """evaluate.box_match_numpy on the rows of every subset alone."""
    hit = np.zeros(qbox.shape[0], np.uint32)
    out = None if payload is None else np.full((S, qbox.shape[0], payload.shape[2]), NEG_INF)
    for s in range(S):
        qi, ki = np.nonzero((qmask >> np.uint32(s)) & np.uint32(1))[0], np.nonzero((kmask >> np.uint32(s)) & np.uint32(1))[0]
        h, o = evaluate.box_match_numpy(qbox[qi], qgroup[qi], kbox[ki], kgroup[ki], None if payload is None else payload[s][ki])
        hit[qi[h]] |= np.uint32(1 << s)
        if out is not None:
            out[s, qi] = o
    return hit, out


@pytest.mark.parametrize("S", [1, 12, 32])
def test_member_restatement_is_the_single_set_one_on_every_subset(S):
    r = np.random.default_rng(S)
    for name in ("blobs_0", "cell_edges", "two_groups"):
        xy, group, eps, _ = CASES[name]
        conf = np.round(r.uniform(0.3, 1.0, xy.shape[0]), 2)
        mask = subset_masks(xy.shape[0], S, 5)
        got = kfold.member_conf_subsets_numpy(xy, group, conf, mask, eps, 6, S)
        assert got.shape == (S, xy.shape[0], 6) and np.array_equal(got, member_by_subset(xy, group, conf, mask, eps, 6, S))
        if S > 1:
            assert (got[0] == NEG_INF).all() and (got[:, :2] == NEG_INF).all()
            full = evaluate.member_conf_numpy(xy[2:], group[2:], conf[2:], eps, 6)
            assert np.array_equal(got[S - 1, 2:], full)
    assert kfold.member_conf_subsets_numpy(np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros(0, np.uint32), 5.0, 3, S).shape == (S, 0, 3)
    with pytest.raises(ValueError):
        kfold.member_conf_subsets_numpy(xy, group, conf, mask, eps, 6, 33)
    with pytest.raises(ValueError):
        kfold.member_conf_subsets_numpy(xy, group, conf, mask, eps, 6, 0)


@pytest.mark.parametrize("S", [1, 12, 32])
def test_join_restatement_is_the_single_set_one_on_every_subset(S):
    r = np.random.default_rng(10 + S)

    def boxes(n):
        a, w = r.integers(0, 40, (n, 2)).astype(np.float64), r.integers(0, 4, (n, 2)).astype(np.float64)
        return np.concatenate([a, a + w], 1)

    q, k = boxes(300), boxes(400)
    qg, kg = r.integers(-1, 5, 300), r.choice([0, 1, 2, 4], 400)
    qm, km = subset_masks(300, S, 1), subset_masks(400, S, 2)
    pay = np.round(r.uniform(0, 1, (S, 400, 5)), 2)
    hit, out = kfold.box_match_subsets_numpy(q, qg, qm, k, kg, km, S, pay)
    want_hit, want_out = match_by_subset(q, qg, qm, k, kg, km, S, pay)
    assert hit.dtype == np.uint32 and np.array_equal(hit, want_hit) and np.array_equal(out, want_out) and np.isfinite(out).any()
    assert (hit & ~qm).max() == 0
    hit2, none = kfold.box_match_subsets_numpy(q, qg, qm, k, kg, km, S)
    assert none is None and np.array_equal(hit2, hit)
    if S > 1:
        assert (hit & 1).max() == 0 and (out[0] == NEG_INF).all() and (hit[:2] == 0).all() and (out[:, :2] == NEG_INF).all()
        all_hit = evaluate.box_match_numpy(q[2:], qg[2:], k[2:], kg[2:])[0]
        assert np.array_equal((hit[2:] >> np.uint32(S - 1)).astype(bool), all_hit)


# ---- the whole procedure against the reference's, literally ----

def rows_of(data, dsel, lsel):
    """The detections dsel and the labels lsel (bool per row) of evaluate.inputs' `data`, cut here and not by the code under test."""
    cut = lambda sample, sel: {k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in sample.items()}
    return {"det": cut(data["det"], dsel), "lab": cut(data["lab"], lsel), "years": data["years"]}


def literal_fold(data, dsel, lsel, tsel, tlsel, grids):
    """get_fold_performance for one fold: the grid on the train detections (dsel) and labels (lsel) with scikit-learn's DBSCAN per grid point
    and year and brute-force joins; the winners by idxmax; their counts on the test detections (tsel) and labels (tlsel).  Each metric uses its
    own threshold on the test set (the deviation kfold.py's docstring names)."""
    import itertools
    import pandas as pd
    train, test = Oracle(rows_of(data, dsel, lsel)), Oracle(rows_of(data, tsel, tlsel))
    combos = list(itertools.product(*(v.tolist() for v in grids)))
    counts = [train.counts(c, e, m) for c, e, m in combos]
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.array([c[1] / c[0] if c[0] else np.nan for c in counts])
        r = np.array([c[3] / c[2] if c[2] else np.nan for c in counts])
        results = pd.DataFrame({"precision": p, "recall": r})
        results["product"] = results["precision"] * results["recall"]
        results["f_score"] = 2 * (results["product"] / (results["precision"] + results["recall"]))
    out = []
    for metric in ("product", "f_score"):
        k = int(results[metric].idxmax())
        out.append((combos[k], test.counts(*combos[k]), counts, float(results[metric][k])))
    return out


@pytest.mark.parametrize("N", [3, 5])
def test_cross_validation_equals_the_references_procedure_fold_by_fold(N):
    data, images, names = fixture_images()
    assert_no_near_ties(data, SMALL_GRID[1])
    split = kfold.split_images(images["bucket"], N, 1, 0.1)
    assert (split < 0).sum() == 8 and sorted(set(split.tolist())) == [-1] + list(range(N))
    res = evaluate.cross_validate(data, images, split, N, *SMALL_GRID, op=(0.785, 50.0, 5), cpu=True)
    assert len(res["rows"]) == 2 * N and [r["fold_id"] for r in res["rows"]] == [f for f in range(N) for _ in range(2)]
    assert [r["metric"] for r in res["rows"]] == ["product", "f_score"] * N
    det_split, lab_split = split[images["det_row"]], split[images["lab_row"]]
    crossing = 0
    for f in range(N):
        dtr, ltr = (det_split >= 0) & (det_split != f), (lab_split >= 0) & (lab_split != f)
        lit = literal_fold(data, dtr, ltr, det_split == f, lab_split == f, SMALL_GRID)
        t = res["tables"][f]
        got = list(zip(t["n_pred"].tolist(), t["n_pred_tp"].tolist(), t["n_label"].tolist(), t["n_label_tp"].tolist()))
        assert got == lit[0][2], f                          # every count of the fold's grid
        for j, ((combo, test_counts, _, score), row) in enumerate(zip(lit, res["rows"][2 * f:2 * f + 2])):
            assert (row["train_best_conf_thresh"], row["train_best_distance_threshold"], row["train_best_min_cluster_size"]) == combo, (f, j)
            assert (row["test_n_pred"], row["test_n_pred_tp"], row["test_n_label"], row["test_n_label_tp"]) == test_counts, (f, j)
            assert row["train_score"] == score and row["test_precision"] == test_counts[1] / test_counts[0] and row["test_recall"] == test_counts[3] / test_counts[2]
        # a join over all images would count pairs the fold does not hold
        whole = Oracle(data)
        crossing += int((whole.meet[dtr][:, ~ltr].any(1) & ~whole.meet[dtr][:, ltr].any(1)).sum())
    assert crossing > 0
    held_d, held_l = det_split < 0, lab_split < 0
    want = Oracle(rows_of(data, held_d, held_l)).counts(0.785, 50.0, 5)
    cage = res["holdout"]["cage"]
    assert (cage["n_pred"], cage["n_pred_tp"], cage["n_label"], cage["n_label_tp"]) == want and want[2] > 0


def test_fold_grid_is_evaluate_grid_on_the_folds_images():
    """The batched grid phase against the path the parent commit has: evaluate.grid per fold through an image list."""
    data, images, names = fixture_images()
    split = kfold.split_images(images["bucket"], 3, 1, 0.1)
    res = evaluate.cross_validate(data, images, split, 3, *SMALL_GRID, cpu=True)
    for f in range(3):
        fold_names = [n for n, s in zip(names, split) if s >= 0 and s != f]
        want = evaluate.grid(evaluate.inputs(detection_table(), truth(), images=fold_names), *SMALL_GRID, cpu=True)
        for c in evaluate.COLUMNS:
            assert np.array_equal(res["tables"][f][c], want[c], equal_nan=True), (f, c)
    assert res["holdout"] is None


# ---- the surface ----

def test_symbols_are_declared_exported_and_bound(lib):
    import ctypes
    from aquaculture_amd import build, engine
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    for name in ("aq_eval_subsets_scratch_bytes", "aq_eval_member_conf_subsets_f64", "aq_box_match_subsets_scratch_bytes", "aq_box_match_subsets_f64"):
        assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert callable(engine.eval_member_conf_subsets) and callable(engine.box_match_subsets)
    assert lib.aq_eval_subsets_scratch_bytes.restype is ctypes.c_size_t
    sb = lib.aq_eval_subsets_scratch_bytes
    assert sb(0, 4, 2) == 0 and sb(1 << 31, 4, 2) == 0 and sb(1000, 0, 2) == 0 and sb(1000, 17, 2) == 0 and sb(1000, 4, 0) == 0 and sb(1000, 4, 33) == 0
    assert sb(1000, 10, 12) == 16000 + 24000 + 8000 + 4000 + 80000 * 12
    assert sb(1001, 1, 1) == 16016 + 24032 + 8016 + 4016 + 8016
    assert sb((1 << 27) - 1, 16, 32) > 0 and sb(1 << 27, 16, 32) == 0       # S n K = 2^36
    mb = lib.aq_box_match_subsets_scratch_bytes
    assert sb(10, (1 << 31) - 1, (1 << 31) - 1) == 0 and mb(10, 10, (1 << 31) - 1, (1 << 31) - 1) != 0      # no product is formed from these
    assert mb(10, 10, 0, 1) == 0 and mb(10, 10, 16, 32) == 0 and mb(10, 1 << 31, 0, 1) != 0 and mb(1 << 27, 10, 16, 32) != 0 and mb(10, 10, 0, 33) != 0
    assert engine.EVAL_MAX_S == kfold.MAX_SUBSETS == 32
    assert ("eval_subsets.hip", ["-ffp-contract=off"]) in build.SOURCES
    src = open(os.path.join(ROOT, "aquaculture_amd", "csrc", "eval_subsets.hip")).read()
    guards = open(os.path.join(ROOT, "aquaculture_amd", "csrc", "size_guards.h")).read()
    assert "inline bool eval_subsets_fit(" in guards and src.count("sg::eval_subsets_fit(") >= 5


def test_options_and_refusals():
    from aquaculture_amd import detect
    base = ["--evaluate", "truth.geojson", "--geocode-bboxes", "wb.csv"]
    opt = detect.parse_opt(base)
    assert (opt.evaluate_kfold, opt.evaluate_kfold_images, opt.evaluate_known_sites, opt.evaluate_kfold_seed, opt.evaluate_kfold_test) == (None, None, None, 1, 0.1)
    assert detect.parse_opt(base + ["--evaluate-kfold"]).evaluate_kfold == 5
    opt = detect.parse_opt(base + ["--evaluate-kfold", "3", "--evaluate-kfold-seed", "7", "--evaluate-kfold-test", "0", "--evaluate-known-sites", "s.csv",
                                   "--evaluate-kfold-images", "i.txt"])
    assert (opt.evaluate_kfold, opt.evaluate_kfold_images, opt.evaluate_known_sites, opt.evaluate_kfold_seed, opt.evaluate_kfold_test) == (3, "i.txt", "s.csv", 7, 0.0)
    for bad in (["--evaluate-kfold", "3"], base + ["--evaluate-kfold", "1"], base + ["--evaluate-kfold", "16"], base + ["--evaluate-kfold", "3", "--evaluate-kfold-test", "1"]):
        with pytest.raises(SystemExit):
            detect.parse_opt(bad)
    with pytest.raises(ValueError, match="--evaluate TRUTH_GEOJSON"):
        detect.run("w.pt", "src", evaluate_kfold=5)
    with pytest.raises(ValueError, match="2 to 15"):
        detect.run("w.pt", "src", evaluate="t.geojson", geocode_bboxes="wb.csv", evaluate_kfold=16)
    # scene mode lists its tiles nowhere after the sweep: the image table then has to be named
    with pytest.raises(SystemExit):
        detect.parse_opt(base + ["--evaluate-kfold", "--tile-scenes"])
    with pytest.raises(ValueError, match="--evaluate-kfold-images FILE"):
        detect.run("w.pt", "src", evaluate="t.geojson", geocode_bboxes="wb.csv", evaluate_kfold=5, tile_scenes=1024)
    opt = detect.parse_opt(base + ["--evaluate-kfold", "--tile-scenes", "--evaluate-kfold-images", "i.txt"])
    assert opt.tile_scenes and opt.evaluate_kfold == 5 and opt.evaluate_kfold_images == "i.txt"
    assert not detect.parse_opt(base + ["--tile-scenes"]).evaluate_kfold                                     # scene mode alone is untouched
    assert "evaluate_kfold" not in detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True)      # --resume: as the other --evaluate-* options
    with pytest.raises(SystemExit):
        evaluate.main(["--labels", "l", "--geocode-bboxes", "wb.csv", "--truth", "t.geojson", "--evaluate-kfold", "40"])


def test_without_the_flag_two_files_with_it_three_more_that_round_trip(tmp_path):
    truth_path = write_truth_geojson(str(tmp_path / "truth.geojson"))
    plain = str(tmp_path / "plain")
    evaluate.evaluate_table(detection_table(), truth_path, plain, *SMALL_GRID, op=(0.785, 50.0, 5), cpu=True)
    assert sorted(os.listdir(plain)) == [evaluate.CSV_FILE, evaluate.JSON_FILE]
    names, rects, sites = kfold_inputs()
    out = str(tmp_path / "kfold")
    s = evaluate.kfold(detection_table(), truth(), out, 3, names=names, rects=rects, sites=sites, conf_grid=SMALL_GRID[0], eps_grid=SMALL_GRID[1],
                       min_grid=SMALL_GRID[2], op=(0.785, 50.0, 5), cpu=True)
    assert sorted(os.listdir(out)) == sorted(evaluate.KFOLD_FILES) == sorted([kfold.RESULTS_FILE, kfold.IMAGES_FILE, kfold.JSON_FILE])
    text = open(os.path.join(out, kfold.JSON_FILE)).read()
    assert "NaN" not in text and json.loads(text) == s and s["device"] == "cpu" and s["parameters"]["seed"] == 1 and s["parameters"]["n_splits"] == 3
    assert s["n_images"] == 78 and s["n_test_images"] == 8 and [b["bucket"] for b in s["strata"]] == list(kfold.STRATA)
    assert s["holdout"]["cage"]["n_label"] > 0 and set(s["folds"]) == {"product", "f_score"}
    lines = open(os.path.join(out, kfold.RESULTS_FILE)).read().splitlines()
    assert lines[0] == ",".join(kfold.RESULT_COLUMNS) and lines[0].startswith("test_precision,test_recall,train_best_conf_thresh,train_best_distance_threshold,"
                                                                               "train_best_min_cluster_size,metric,fold_id,") and len(lines) == 7
    data, images, _ = fixture_images()
    split = kfold.split_images(images["bucket"], 3, 1, 0.1)
    res = evaluate.cross_validate(data, images, split, 3, *SMALL_GRID, op=(0.785, 50.0, 5), cpu=True)
    assert kfold.read_results_csv(os.path.join(out, kfold.RESULTS_FILE)) == res["rows"]
    prec = np.array([r["test_precision"] for r in res["rows"] if r["metric"] == "f_score"])
    assert s["folds"]["f_score"]["test_precision"] == {"folds": 3, "mean": float(prec.mean()), "sd": float(prec.std(ddof=1))}
    back = kfold.read_images_csv(os.path.join(out, kfold.IMAGES_FILE))
    assert back["image"] == names and back["split"] == kfold.split_names(split) and back["n_detections"] == images["n_detections"].tolist()
    assert back["bucket"] == [kfold.STRATA[b] for b in images["bucket"]] and back["in_known_area"] == images["in_known_area"].tolist()
    assert np.array_equal(back["det_conf"], images["det_conf"], equal_nan=True) and back["year"] == images["year"].tolist()
    assert open(os.path.join(out, kfold.IMAGES_FILE)).readline().strip() == ",".join(kfold.IMAGE_COLUMNS)
    # a fold without a winner: empty cells
    empty = {c: None for c in kfold.RESULT_COLUMNS}
    empty.update(metric="product", fold_id=0)
    kfold.write_results_csv(str(tmp_path / "e.csv"), [empty])
    assert open(str(tmp_path / "e.csv")).read().splitlines()[1] == ",,,,,product,0,,,,,"
    # the default table: the images with a detection or a label; --evaluate-images restricts it
    s2 = evaluate.kfold(detection_table(), truth(), str(tmp_path / "k2"), 2, conf_grid=SMALL_GRID[0], eps_grid=SMALL_GRID[1], min_grid=SMALL_GRID[2],
                        images=names[:30], cpu=True, test_frac=0)
    assert s2["n_images"] == 30 and s2["n_test_images"] == 0 and s2["holdout"] is None
