"""--tonnage without a GPU: the numpy restatement (aquaculture_amd/tonnage.py) that csrc/tonnage.hip equals bit for bit
(tests/test_gpu_tonnage.py).  Philox known answers, the arithmetic-only ndtri against scipy, the sampler against a literal restatement
of the reference's loop (numpy / scipy generators with the reference's arguments), exact bookkeeping of the bounds, the resampling
path, chunk invariance, the input files and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def test_philox_known_answers():
    from aquaculture_amd import tonnage
    for counter, key, want in KAT:
        got = tonnage.philox4x32(*(np.array([c]) for c in counter), key[0], key[1])
        assert tuple(int(w[0]) for w in got) == want
    # whole arrays at once give the same words, and the uniform is built from words 0 and 1
    cs = np.array([k[0] for k in KAT[:1] * 3], np.uint64)
    w = tonnage.philox4x32(cs[:, 0], cs[:, 1], cs[:, 2], cs[:, 3], 0, 0)
    assert [int(v) for v in w[0]] == [KAT[0][2][0]] * 3
    u = tonnage.uniform(0, 0, 0, 0, 0)
    assert float(u) == (float(((KAT[0][2][1] << 32) | KAT[0][2][0]) >> 11) + 0.5) * 2.0 ** -53
    # strictly inside (0, 1) at both ends of the word range (x + 0.5 rounds to 2^53 at the top; the selection keeps it below 1)
    assert 0.0 < float(tonnage.uniform_from_words(np.uint64(0), np.uint64(0))) == 2.0 ** -54
    assert float(tonnage.uniform_from_words(np.uint64(0xffffffff), np.uint64(0xffffffff))) == 1.0 - 2.0 ** -53


def ndtri_points():
    """The point set of the ndtri tests (the GPU test takes the same)."""
    e2 = 0.13533528323661269189
    pts = [2.0 ** -54, 1 - 2.0 ** -54, np.nextafter(e2, 0), e2, np.nextafter(e2, 1), np.nextafter(1 - e2, 0), 1 - e2, np.nextafter(1 - e2, 1),
           1.2e-14, 1.3e-14, 0.5]
    u = np.random.default_rng(11).random(2_000_000)
    lg = 10.0 ** np.random.default_rng(12).uniform(-300.0, -1.0, 500_000)
    return np.concatenate([np.asarray(pts), u[(u > 0) & (u < 1)], lg])


def test_ndtri_against_scipy():
    from scipy.special import ndtri
    from aquaculture_amd import tonnage
    p = ndtri_points()
    got, want = tonnage.ndtri(p), ndtri(p)
    # 1 - 2^-54 is no fp64 number: it is 1.0, where both sides give +inf; every other point is finite on both sides
    assert p[1] == 1.0 and got[1] == want[1] == np.inf
    got, want = np.delete(got, 1), np.delete(want, 1)
    err = np.abs(got - want)
    print(f"ndtri: max |dz| = {err.max():.3e} over {p.shape[0]} points; relative for |z| >= 1e-3: {(err / np.abs(want))[np.abs(want) >= 1e-3].max():.3e}")
    assert np.isfinite(got).all() and np.isfinite(want).all() and err.max() <= 1e-12
    edge = tonnage.ndtri(np.array([0.0, 1.0, -0.1, 1.1, np.nan]))
    assert edge[0] == -np.inf and edge[1] == np.inf and np.isnan(edge[2:]).all()
    x = np.exp(np.random.default_rng(13).uniform(-700, 700, 200_000))
    assert np.abs(tonnage.alog(x) / np.log(x) - 1).max() < 1e-15
    assert tonnage.alog(np.array([5e-324]))[0] == pytest.approx(np.log(5e-324), rel=1e-15)    # a subnormal


# ---- the sampler is the reference's ----

PASSES = ("2013-2015", "2016-2018")
FACTORS = {"2013-2015": (12.0, 3.0, 0.8, 0.1), "2016-2018": (15.0, 4.0, 0.7, 0.15)}
MIN_DEPTH, MIX = 1.0, 0.5


def small_table():
    """Six facilities over two passes: all three cage kinds, nonzero error sd, facility 2 with an empty min selection, facility 4 with a
    cage only in the max selection.  -> (make_table's dict, a plain description for the reference loop)."""
    from aquaculture_amd import tonnage as tn
    rng = np.random.default_rng(5)
    sizes = (5, 7, 6, 9, 5, 12)
    pass_id = (0, 0, 0, 1, 1, 1)
    depth = (4.84, 6.0, 3.0, 4.84, 9.5, 2.2)
    start, area, kind, sel, mean, sd = [0], [], [], [], [], []
    for f, n in enumerate(sizes):
        for j in range(n):
            k = (f + j) % 3
            kind.append(k)
            area.append(float(rng.uniform(60.0, 400.0)))
            s = tn.SEL_MIN | tn.SEL_MAX | tn.SEL_RANDOM
            if f == 2:
                s = tn.SEL_MAX | tn.SEL_RANDOM
            if f == 4 and j == 1:
                s = tn.SEL_MAX
            sel.append(s)
            mean.append((-4.0, 2.0, 5.0)[k] + pass_id[f])
            sd.append((25.0, 40.0, 30.0)[k])
        start.append(len(area))
    params = tn.pass_params(*([FACTORS[p][j] for p in PASSES] for j in range(4)))
    return tn.make_table(start, area, mean, sd, kind, sel, depth, pass_id, params, MIX, MIN_DEPTH)


def reference_loop(t, K, seed):
    """The reference's loop (src/utils_tonnage.py:57-113 with sample_model_errors :385-451), restated on arrays: the same generator calls
    with the same arguments, per simulation; the facility sums via np.add.at."""
    from scipy.stats import truncnorm
    from aquaculture_amd import tonnage as tn
    np.random.seed(seed)
    F = t["depth"].shape[0]
    fac_of = np.repeat(np.arange(F), np.diff(t["entry_start"]))
    kind, fl = t["flags"] & 3, t["flags"]
    a0, mean, sd = t["area"], t["err"][:, 0], t["err"][:, 1]
    d = t["depth"]
    q = t["params"][t["pass_id"]]
    s_mean, s_sd, h_mean, h_sd = q[:, 0], q[:, 1], q[:, 4], q[:, 5]
    T = np.zeros((K, t["params"].shape[0]))
    for k in range(K):
        area = a0 + np.random.normal(loc=mean, scale=sd)
        while area.min() <= 0:
            err = np.random.normal(loc=mean, scale=sd)
            area = np.where(area <= 0, a0 + err, area)
        mn = np.where(kind == 0, area, np.where(kind == 1, 4 * area / (2 + np.pi), 2 * area / 3))
        mx = np.where(kind == 0, area, np.where(kind == 1, 2 * np.pi * area / (2 + np.pi), 4 * area / 3))
        lo, hi = np.zeros(F), np.zeros(F)
        np.add.at(lo, fac_of[(fl & tn.SEL_MIN) != 0], mn[(fl & tn.SEL_MIN) != 0])
        np.add.at(hi, fac_of[(fl & tn.SEL_MAX) != 0], mx[(fl & tn.SEL_MAX) != 0])
        sim_area = np.random.uniform(low=lo, high=hi)
        bern = np.random.binomial(n=1, p=t["mix"], size=F)
        dA = truncnorm.rvs(loc=d, scale=(d - MIN_DEPTH) / 1.96, a=(MIN_DEPTH - d) / ((d - MIN_DEPTH) / 1.96), b=0)
        dB = truncnorm.rvs(loc=d, scale=d / 1.96, a=0, b=d / (d / 1.96))
        depth = np.where(bern == 1, dA, dB)
        stock = truncnorm.rvs(loc=s_mean, scale=s_sd, a=(5 - s_mean) / s_sd, b=(20 - s_mean) / s_sd)
        harvest = np.random.normal(loc=h_mean, scale=h_sd)
        ton = sim_area * depth * stock
        ton *= harvest * (1 / 1000)
        np.add.at(T[k], t["pass_id"], ton)
    return T


def test_sampler_is_the_references():
    from aquaculture_amd import tonnage as tn
    t = small_table()
    K = 4000
    ours = tn.simulate(t, K, seed=2024, cpu=True)["T"]
    ref = reference_loop(t, K, seed=7)
    for p in range(len(PASSES)):
        m1, m2, s1, s2 = ours[:, p].mean(), ref[:, p].mean(), ours[:, p].std(), ref[:, p].std()
        se_mean = np.sqrt(s1 * s1 / K + s2 * s2 / K)
        se_sd = np.sqrt(s1 * s1 / (2 * K) + s2 * s2 / (2 * K))
        print(f"pass {p}: tonnage {m1:.4f} vs {m2:.4f} ({abs(m1 - m2) / se_mean:.2f} se), sd {s1:.4f} vs {s2:.4f} ({abs(s1 - s2) / se_sd:.2f} se)")
        assert abs(m1 - m2) <= 5 * se_mean
        assert abs(s1 - s2) <= 5 * se_sd


def test_marginal_draws_follow_their_distributions():
    """Kolmogorov-Smirnov, K = 10000 draws, seed 3 (the first seed tried): the uniform area, the two depth branches, the stocking
    density and the harvest frequency, each recovered from a one-facility table in which everything else is fixed."""
    from scipy import stats
    from aquaculture_amd import tonnage as tn
    K, seed = 10000, 3
    ks = np.arange(K, dtype=np.uint64)
    d, m = 6.0, 1.0
    pr = tn.depth_probs()
    u = lambda slot: tn.uniform(seed, ks, 0, slot, 0)
    draws = {
        "area": (100.0 + (300.0 - 100.0) * u(tn.SLOT_AREA), stats.uniform(loc=100.0, scale=200.0)),
        "depth A": (d + ((d - m) / 1.96) * tn.ndtri(pr[0] + u(tn.SLOT_DEPTH_A) * (pr[1] - pr[0])),
                    stats.truncnorm(loc=d, scale=(d - m) / 1.96, a=(m - d) / ((d - m) / 1.96), b=0)),
        "depth B": (d + (d / 1.96) * tn.ndtri(pr[2] + u(tn.SLOT_DEPTH_B) * (pr[3] - pr[2])), stats.truncnorm(loc=d, scale=d / 1.96, a=0, b=1.96)),
        "harvest": (0.8 + 0.1 * tn.ndtri(u(tn.SLOT_HARVEST)), stats.norm(loc=0.8, scale=0.1)),
    }
    q = tn.pass_params([12.0], [3.0], [0.8], [0.1])[0]
    draws["stocking"] = (q[0] + q[1] * tn.ndtri(q[2] + u(tn.SLOT_STOCKING) * (q[3] - q[2])), stats.truncnorm(loc=12.0, scale=3.0, a=(5 - 12.0) / 3.0, b=(20 - 12.0) / 3.0))
    for name, (x, dist) in draws.items():
        pv = stats.kstest(x, dist.cdf).pvalue
        print(f"{name}: KS p = {pv:.4f}")
        assert pv > 1e-3, name
    share = float((u(tn.SLOT_BERNOULLI) < 0.3).mean())
    assert abs(share - 0.3) < 5 * np.sqrt(0.3 * 0.7 / K)
    # and the simulation uses exactly these draws: one facility of one full-ellipse cage without model error
    t = tn.make_table([0, 1], [250.0], [0.0], [0.0], [tn.KIND_FULL], [tn.SEL_MIN | tn.SEL_MAX], [d], [0], q[None, :], 0.3, m)
    ton = tn.simulate_numpy(t, 64, seed)[:, 0]
    depth = np.where(u(tn.SLOT_BERNOULLI) < 0.3, draws["depth A"][0], draws["depth B"][0])[:64]
    assert np.array_equal(ton, ((250.0 * depth) * draws["stocking"][0][:64]) * (draws["harvest"][0][:64] * (1 / 1000)))


# ---- exact bookkeeping ----

def test_bounds_are_the_sequential_sums_by_kind():
    """Without model error lo and hi are the sums, one after the other in entry order, of the cages' bounds by kind -- which are
    facilities._areas' min_area and max_area up to the rounding of going through the area estimate."""
    from aquaculture_amd import facilities, tonnage as tn
    rng = np.random.default_rng(8)
    n = 40
    w, h = rng.uniform(5, 30, n), rng.uniform(5, 30, n)
    circle = np.arange(n) % 3 != 2
    xb, yb = (np.arange(n) % 3 == 1) & (np.arange(n) % 2 == 0), (np.arange(n) % 3 == 1) & (np.arange(n) % 4 != 0)
    a = facilities._areas(w, h, circle, ~circle, xb, yb)
    kind = np.where(~circle, tn.KIND_SQUARE, np.where(a["area_var"] == 0.0, tn.KIND_FULL, tn.KIND_BORDER))
    assert set(kind.tolist()) == {0, 1, 2}
    start = [0, 1, 14, 14, 40]                              # one cage, thirteen, none, twenty-six
    sel = np.full(n, tn.SEL_MIN | tn.SEL_MAX)
    sel[20:24] = tn.SEL_MAX
    t = tn.make_table(start, a["area"], np.zeros(n), np.zeros(n), kind, sel, [5.0] * 4, [0] * 4, tn.pass_params([12.0], [3.0], [0.8], [0.1]))
    st = {}
    tn.simulate_numpy(t, 3, 1, stats=st)
    area = a["area"]
    mn = np.where(kind == 1, (4.0 * area) / (2.0 + np.pi), np.where(kind == 2, (2.0 * area) / 3.0, area))
    mx = np.where(kind == 1, ((2.0 * np.pi) * area) / (2.0 + np.pi), np.where(kind == 2, (4.0 * area) / 3.0, area))
    for f in range(4):
        lo = hi = lo_a = hi_a = 0.0
        for e in range(start[f], start[f + 1]):
            if sel[e] & tn.SEL_MIN:
                lo, lo_a = lo + mn[e], lo_a + a["min_area"][e]
            hi, hi_a = hi + mx[e], hi_a + a["max_area"][e]
        assert (st["lo"][:, f] == lo).all() and (st["hi"][:, f] == hi).all()
        assert lo == pytest.approx(lo_a, rel=1e-14) and hi == pytest.approx(hi_a, rel=1e-14)
    assert (st["lo"][:, 2] == 0).all() and st["draws"][0] == 0 and st["capped"] == 0


def resampling_table(n=64):
    """Entries of area 1 under an error of sd 50: about half of the first draws are not positive."""
    from aquaculture_amd import tonnage as tn
    return tn.make_table([0, n], np.ones(n), np.zeros(n), np.full(n, 50.0), np.arange(n) % 3, np.full(n, tn.SEL_MIN | tn.SEL_MAX), [5.0], [0],
                         tn.pass_params([12.0], [3.0], [0.8], [0.1]))


def test_resampling_path():
    from aquaculture_amd import tonnage as tn
    t = resampling_table()
    st = {}
    ton = tn.simulate_numpy(t, 16, 5, stats=st)
    assert st["draws"][0] >= 100 and st["draws"][1] >= 1, st["draws"][:4]
    assert st["min_area"] > 0 and st["capped"] == 0 and (st["lo"] > 0).all() and np.isfinite(ton).all()
    # the cap: an error that can never make the area positive leaves area_orig after 64 draws
    t2 = tn.make_table([0, 1], [1.0], [-1e6], [1.0], [0], [tn.SEL_MIN | tn.SEL_MAX], [5.0], [0], tn.pass_params([12.0], [3.0], [0.8], [0.1]))
    st2 = {}
    tn.simulate_numpy(t2, 2, 5, stats=st2)
    assert st2["capped"] == 2 and st2["draws"][62] == 2 and (st2["lo"] == 1.0).all()


def test_chunks_change_no_byte():
    from aquaculture_amd import tonnage as tn
    t = small_table()
    whole = tn.simulate(t, 257, seed=9, cpu=True, chunk=257, keep_ton=True)
    parts = tn.simulate(t, 257, seed=9, cpu=True, chunk=100, keep_ton=True)
    assert tn.chunk_sizes(257, 6, 100) == [100, 100, 57]
    for k in ("ton", "T", "moments"):
        assert whole[k].tobytes() == parts[k].tobytes(), k
    # k0 is the only thing a later chunk knows of the earlier ones
    assert np.array_equal(tn.simulate_numpy(t, 57, 9, 200), whole["ton"][200:])
    assert not np.array_equal(tn.simulate_numpy(t, 57, 10, 200), whole["ton"][200:])
    # the pass sums and the moments are the sequential sums
    T = np.zeros((257, 2))
    for f in range(6):
        T[:, t["pass_id"][f]] += whole["ton"][:, f]
    assert np.array_equal(T, whole["T"])
    s = 0.0
    for k in range(257):
        s = s + whole["ton"][k, 3]
    assert s == whole["moments"][3, 0]


# ---- files and command line ----

def test_symbols_are_declared_exported_and_bound(lib):
    import ctypes
    from aquaculture_amd import build, engine
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    for name in ("aq_tonnage_simulate_f64", "aq_tonnage_reduce_f64", "aq_tonnage_ndtri_f64", "aq_tonnage_uniform_f64"):
        assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
        assert getattr(lib, name).restype is ctypes.c_int
    assert ("tonnage.hip", ["-ffp-contract=off"]) in build.SOURCES
    # refusals that need no GPU: nothing is launched before the arguments are checked
    assert lib.aq_tonnage_ndtri_f64(None, 1 << 31, None, None) != 0 and lib.aq_tonnage_ndtri_f64(None, 5, None, None) != 0
    assert lib.aq_tonnage_ndtri_f64(None, 0, None, None) == 0
    assert lib.aq_tonnage_simulate_f64(0, 0, 0, None, None, 0, None, None, None, 0, None, None, None, None, 0, 0.5, 1.0, None, None, None) == 0
    assert lib.aq_tonnage_simulate_f64(0, 0, 0, None, None, 0, None, None, None, 0, None, None, None, None, 0, 1.5, 1.0, None, None, None) != 0
    assert b"mix" in lib.aq_last_error()


def synthetic_run(tmp_path):
    """A label directory and a bounds table laid out for exactly two facilities and some noise, made as tests/test_facilities.py lays its
    cages out: scene 3 is 1843.2 m wide in EPSG:3857 (0.3 m per pixel); tile (0, 0) of 2015 holds six circles 12 px apart, one of them at
    the image's left border (a border ellipse), and a stray square; tile (1024, 0) five squares, a stray circle and a circle of low
    confidence among the squares; the same tile of 2012 three circles (too few)."""
    from aquaculture_amd import geocode
    labels = tmp_path / "labels"
    labels.mkdir()
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.5), np.float64(43.3)))
    csv_path = tmp_path / "wanted_bboxes.csv"
    x1, y1 = x0 + 1843.2, y0 + 1843.2
    with open(csv_path, "w") as f:
        f.write(",geometry\n")
        f.write(f'3,"POLYGON (({x1!r} {y0!r}, {x1!r} {y1!r}, {x0!r} {y1!r}, {x0!r} {y0!r}, {x1!r} {y0!r}))"\n')
    row = lambda cls, px, py, w, conf: f"{cls} {px / 1024:g} {py / 1024:g} {w / 1024:g} {w / 1024:g} {conf:g}\n"
    files = {"ORTHOIMAGERY.ORTHOPHOTOS2015_3_0_0": [row(0, 5 + 12 * k, 500, 10, 0.9) for k in range(6)] + [row(1, 800, 100, 10, 0.9)],
             "ORTHOIMAGERY.ORTHOPHOTOS2015_3_1024_0": [row(1, 300 + 12 * k, 200 + 5 * (k % 2), 10, 0.8) for k in range(5)]
                                                      + [row(0, 900, 900, 10, 0.9), row(0, 318, 212, 10, 0.3)],
             "ORTHOIMAGERY.ORTHOPHOTOS2012_3_1024_0": [row(0, 300 + 12 * k, 200, 10, 0.9) for k in range(3)]}
    for stem, rows in files.items():
        (labels / (stem + ".txt")).write_text("".join(rows))
    return str(labels), str(csv_path)


def write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_input_files_and_their_refusals(tmp_path):
    from aquaculture_amd import tonnage as tn
    good = write(tmp_path / "f.csv", "pass,s_mean,s_sd,h_mean,h_sd,species\n2013-2015,12,3,0.8,0.1,bass\n2016-2018,15.5,4,0.7,0.15,bream\n")
    assert tn.read_factors(good) == {"2013-2015": (12.0, 3.0, 0.8, 0.1), "2016-2018": (15.5, 4.0, 0.7, 0.15)}
    js = write(tmp_path / "f.json", json.dumps([{"pass": "2013-2015", "s_mean": 12, "s_sd": 3, "h_mean": 0.8, "h_sd": 0.1}]))
    assert tn.read_factors(js) == {"2013-2015": (12.0, 3.0, 0.8, 0.1)}
    for text, match in (("pass,s_mean,s_sd,h_mean\n2013-2015,12,3,0.8\n", "lacks h_sd"), ("pass,s_mean,s_sd,h_mean,h_sd\n", "no pass"),
                        ("pass,s_mean,s_sd,h_mean,h_sd\na,12,0,0.8,0.1\n", "positive"), ("pass,s_mean,s_sd,h_mean,h_sd\na,nan,1,0.8,0.1\n", "finite"),
                        ("pass,s_mean,s_sd,h_mean,h_sd\na,x,1,0.8,0.1\n", "finite"), ("pass,s_mean,s_sd,h_mean,h_sd\na,1,1,1,-1\n", "negative"),
                        ("pass,s_mean,s_sd,h_mean,h_sd\na,1,1,1,1\na,1,1,1,1\n", "twice")):
        with pytest.raises(ValueError, match=match):
            tn.read_factors(write(tmp_path / "bad.csv", text))
    with pytest.raises(ValueError, match="list of objects"):
        tn.read_factors(write(tmp_path / "bad.json", "{}"))
    e = write(tmp_path / "e.csv", "pass,farm_type,model_error_mean,model_error_sd\n2013-2015,circle_farm,-3.5,20\n2013-2015,square_farm,4,30\n")
    assert tn.read_errors(e) == {("2013-2015", "circle_farm"): (-3.5, 20.0), ("2013-2015", "square_farm"): (4.0, 30.0)}
    for text, match in (("pass,farm_type,model_error_mean,model_error_sd\na,triangle,0,1\n", "farm_type"),
                        ("pass,farm_type,model_error_mean,model_error_sd\na,circle_farm,0,-1\n", "negative"),
                        ("pass,farm_type,model_error_mean,model_error_sd\na,circle_farm,0,1\na,circle_farm,0,1\n", "twice")):
        with pytest.raises(ValueError, match=match):
            tn.read_errors(write(tmp_path / "bad.csv", text))
    d = write(tmp_path / "d.csv", "facility_index,cage_depth\n1,7.5\n0,0.2\n")
    assert tn.read_depths(d) == {1: 7.5, 0: 0.2}
    for text, match in (("facility_index,cage_depth\nx,1\n", "facility_index"), ("facility_index,cage_depth\n1,inf\n", "finite"),
                        ("facility_index,cage_depth\n1,2\n1,2\n", "twice")):
        with pytest.raises(ValueError, match=match):
            tn.read_depths(write(tmp_path / "bad.csv", text))
    with pytest.raises(ValueError, match="probability"):
        tn.make_table([0], [], [], [], [], [], [], [], np.zeros((0, 6)), mix=1.5)
    with pytest.raises(ValueError, match="non-decreasing"):
        tn.make_table([0, 2, 1], [1.0, 1.0], [0, 0], [0, 0], [0, 0], [12, 12], [5.0, 5.0], [0, 0], tn.pass_params([12.0], [3.0], [0.8], [0.1]))


def test_estimate_builds_the_entries_from_the_facility_table():
    from test_facilities import FIVE, LATER, ROW6, hand_table
    from aquaculture_amd import facilities, tonnage as tn
    t = hand_table()
    fac = facilities.cluster(t, "pass", labels_fn=facilities.dbscan_numpy)
    factors = {"2013-2015": (12.0, 3.0, 0.8, 0.1)}
    errors = {("2013-2015", "square_farm"): (2.0, 5.0)}
    tab, passes = tn.build_table(fac, None, t, factors, errors, {1: 0.3}, 0.5, 1.0, 4.84)
    assert passes == ["2013-2015"]
    # facility 1: the rectangle (10) and the triangle (11) have no area estimate and take no part
    assert tab["entry_start"].tolist() == [0, 6, 6 + 3 + 5] and tab["cage_ids"].tolist() == ROW6 + FIVE[:3] + LATER
    assert (tab["flags"][:6] == (tn.KIND_FULL | 28)).all() and (tab["flags"][6:] == (tn.KIND_SQUARE | 28)).all()
    assert (tab["err"][:6] == 0).all() and (tab["err"][6:] == (2.0, 5.0)).all()
    assert tab["depth"].tolist() == [4.84, 1.0]             # the listed 0.3 m is raised to the minimum depth
    assert np.array_equal(tab["area"], fac["_areas"]["area"][tab["cage_ids"]])
    # optional selections: a min selection without the first three cages, an empty one
    fac2 = dict(fac, cage_ids_min=[ROW6[3:], []], cage_ids_max=fac["cage_ids"])
    tab2, _ = tn.build_table(fac2, None, t, factors)
    assert tab2["flags"][:6].tolist() == [24] * 3 + [28] * 3 and (tab2["flags"][6:] == (tn.KIND_SQUARE | 24)).all()
    est = tn.estimate(fac2, None, t, factors, K=200, seed=1, cpu=True)
    assert est["pass"] == ["2013-2015"] and est["tonnage"][0] == float(np.mean(est["T"][:, 0])) and est["tonnage_var"][0] == float(np.var(est["T"][:, 0]))
    assert est["tonnage_sd"][0] == float(np.sqrt(est["tonnage_var"][0])) and est["tonnage"][0] > 0
    assert est["facility_tonnage"][0] + est["facility_tonnage"][1] == pytest.approx(est["tonnage"][0], rel=1e-12)
    assert est["facility_cages"] == [6, 8] and all(s > 0 for s in est["facility_tonnage_sd"])
    with pytest.raises(ValueError, match="no factors for pass 2013-2015"):
        tn.build_table(fac, None, t, {"2000-2004": (1, 1, 1, 1)})
    with pytest.raises(ValueError, match="by pass"):
        tn.build_table(facilities.cluster(t, "year", labels_fn=facilities.dbscan_numpy), None, t, factors)


def test_command_line_on_the_cpu_writes_the_same_bytes_twice(tmp_path):
    from aquaculture_amd import detect, tonnage as tn
    labels, csv_path = synthetic_run(tmp_path)
    factors = write(tmp_path / "factors.csv", "pass,s_mean,s_sd,h_mean,h_sd\n2013-2015,12,3,0.8,0.1\n2010-2012,11,2,0.9,0.1\n")
    errors = write(tmp_path / "errors.json", json.dumps([{"pass": "2013-2015", "farm_type": "circle_farm", "model_error_mean": 0.1, "model_error_sd": 2.0}]))
    outs = []
    for name in ("a", "b"):
        out = tmp_path / name
        r = subprocess.run([sys.executable, "-m", "aquaculture_amd.tonnage", "--labels", labels, "--geocode-bboxes", csv_path, "--tonnage-factors", factors,
                            "--tonnage-errors", errors, "--tonnage-K", "300", "--tonnage-seed", "42", "--cpu", "--out", str(out)],
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "2 facilities, 1 passes, K = 300" in r.stdout, r.stdout
        outs.append({f: open(out / f, "rb").read() for f in (tn.ESTIMATES_FILE, tn.FACILITIES_FILE, tn.JSON_FILE)})
    assert outs[0] == outs[1]
    rows = outs[0][tn.ESTIMATES_FILE].decode().splitlines()
    assert rows[0] == "source,pass,tonnage,tonnage_sd" and rows[1].startswith("Model,2013-2015,") and len(rows) == 2
    assert float(rows[1].split(",")[2]) > 0 and repr(float(rows[1].split(",")[2])) == rows[1].split(",")[2]
    assert outs[0][tn.FACILITIES_FILE].decode().splitlines()[0] == "facility_index,pass,cages,tonnage,tonnage_sd"
    doc = json.loads(outs[0][tn.JSON_FILE])
    assert doc["K"] == 300 and doc["seed"] == 42 and doc["cpu"] is True and doc["device"] == "cpu" and doc["mix"] == 0.5
    # detect.py: the option, its defaults and what it needs
    with pytest.raises(SystemExit):
        detect.parse_opt(["--tonnage", "--geocode-bboxes", "wb.csv"])
    with pytest.raises(SystemExit):
        detect.parse_opt(["--tonnage", "--tonnage-factors", "f.csv"])
    with pytest.raises(ValueError, match="--tonnage .*needs --geocode-bboxes"):
        detect.run("w.pt", "src", tonnage="")
    opt = detect.parse_opt(["--tonnage", "--geocode-bboxes", "wb.csv", "--tonnage-factors", "f.csv"])
    assert (opt.tonnage, opt.tonnage_K, opt.tonnage_seed, opt.tonnage_mix, opt.tonnage_default_depth, opt.tonnage_min_depth) == ("", 10000, 0, 0.5, 4.84, 1.0)
    assert "tonnage" not in detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True)
