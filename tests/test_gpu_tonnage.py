"""--tonnage on the GPU: csrc/tonnage.hip against the numpy restatement of aquaculture_amd/tonnage.py, bit for bit -- the two hooks
(uniform draws and ndtri, every branch), the simulation with its pass sums and facility moments, chunking, refusals -- and both command
lines, each in a child process under its own time limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_tonnage import KAT, ndtri_points, resampling_table, synthetic_run, write

from aquaculture_amd import engine, tonnage as tn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_uniform_hook_is_the_restatements(lib):
    rng = np.random.default_rng(21)
    c = rng.integers(0, 1 << 32, (1000, 4), dtype=np.uint64)
    c[0], c[1], c[2] = (0, 0, 0, 0), (0xffffffff,) * 4, KAT[2][0]
    c[3:10, 0] = (1 << 31) + np.arange(7)                   # simulation numbers past 2^31 are plain unsigned words
    dev = torch.from_numpy(c.astype(np.uint32).view(np.int32)).cuda()
    for seed, rows in ((0, (0,)), ((1 << 64) - 1, (1,)), ((KAT[2][1][1] << 32) | KAT[2][1][0], (2,)), (12345678901234567, ())):
        got = engine.tonnage_uniform(seed, dev).cpu().numpy()
        want = tn.uniform(seed, c[:, 0], c[:, 1], c[:, 2], c[:, 3])
        assert np.array_equal(bits(got), bits(want)) and (got > 0).all() and (got < 1).all()
        for r in rows:                                      # the known answers: the top 53 bits of words 1 and 0
            w = KAT[r][2]
            assert 0 <= int(got[r] * 2.0 ** 53) - (((w[1] << 32) | w[0]) >> 11) <= 1      # (x + 0.5 rounds to even from 2^52 on)
    assert engine.tonnage_uniform(0, dev[:0]).shape == (0,)


def test_ndtri_hook_is_the_restatements(lib):
    p = np.concatenate([ndtri_points(), [0.0, 1.0, -0.5, 1.5, np.nan, 5e-324, 1e-310, 2.0 ** -1022], np.random.default_rng(22).random(100_000),
                        10.0 ** np.random.default_rng(23).uniform(-300.0, -1.0, 20_000), 1.0 - 10.0 ** np.random.default_rng(24).uniform(-16.0, -1.0, 20_000)])
    got = engine.tonnage_ndtri(torch.from_numpy(p).cuda()).cpu().numpy()
    want = tn.ndtri(p)
    nan = np.isnan(want)
    assert nan.sum() == 3 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got[~nan]), bits(want[~nan])), np.nonzero(bits(got) != bits(want))[0][:10]
    assert (np.abs(want[~nan & np.isfinite(want)]) >= 8.0).sum() > 1000      # the far tail, and both mirror branches, are in the set
    assert (want[~nan] > 7.0).any() and (want[~nan] < -7.0).any()


# ---- the simulation ----

def params(s=((12.0, 3.0, 0.8, 0.1),)):
    return tn.pass_params(*([row[j] for row in s] for j in range(4)))


def tables():
    rng = np.random.default_rng(31)
    out = {"one": tn.make_table([0, 1], [250.0], [1.0], [20.0], [tn.KIND_BORDER], [tn.SEL_MIN | tn.SEL_MAX], [4.84], [0], params())}
    # 1, 5, 70 and 130 entries; three passes, the middle one empty; d = m and d < m; stocking bounds deep in a tail
    sizes = (1, 5, 70, 130)
    n = sum(sizes)
    sel = np.full(n, tn.SEL_MIN | tn.SEL_MAX | tn.SEL_RANDOM)
    sel[1:6] = tn.SEL_MAX | tn.SEL_RANDOM                   # facility 1: an empty min selection
    sel[6:76:3] = tn.SEL_MAX
    sel[80:90] = tn.SEL_MIN
    sel[100] = tn.SEL_RANDOM
    out["four"] = tn.make_table(np.cumsum((0,) + sizes), rng.uniform(40.0, 500.0, n), rng.uniform(-5.0, 5.0, n), rng.uniform(0.0, 60.0, n),
                                np.arange(n) % 3, sel, [6.0, 1.0, 0.4, 9.25], [0, 2, 2, 0], params(((4.0, 0.5, 0.8, 0.1), (12.0, 3.0, 0.8, 0.1), (21.0, 2.0, 0.7, 0.2))),
                                0.35, 1.0)
    out["resample"] = resampling_table()
    return out


TABLES = tables()
REFERENCE = {}


def reference(name, K, k0):
    """The restatement's results, computed once per case and shared."""
    key = (name, K, k0)
    if key not in REFERENCE:
        t = TABLES[name]
        ton = tn.simulate_numpy(t, K, 77, k0)
        mom = np.zeros((t["depth"].shape[0], 2))
        REFERENCE[key] = (ton, tn.reduce_numpy(ton, t["pass_id"], t["params"].shape[0], mom), mom)
        for a in REFERENCE[key]:
            a.setflags(write=False)
    return REFERENCE[key]


def run_gpu(t, K, k0, chunk=None, seed=77):
    return tn.simulate(t, K, seed, k0, chunk=chunk or K, keep_ton=True)


@pytest.mark.parametrize("k0", [0, (1 << 31) - 300])
@pytest.mark.parametrize("K", [1, 63, 65, 257])
@pytest.mark.parametrize("name", sorted(TABLES))
def test_simulation_is_the_restatements(lib, name, K, k0):
    got = run_gpu(TABLES[name], K, k0)
    ton, T, mom = reference(name, K, k0)
    assert np.array_equal(bits(got["ton"]), bits(ton)), np.argwhere(bits(got["ton"]) != bits(ton))[:5]
    assert np.array_equal(bits(got["T"]), bits(T)) and np.array_equal(bits(got["moments"]), bits(mom))
    assert np.isfinite(ton).all()
    if name == "four":
        assert (T[:, 1] == 0).all() and not np.signbit(got["T"][:, 1]).any()       # the empty pass: +0
        assert K < 63 or (ton[:, 1] != ton[0, 1]).any()


def test_same_bytes_twice_and_in_chunks(lib):
    t = TABLES["four"]
    a, b = run_gpu(t, 257, 0), run_gpu(t, 257, 0)
    c = run_gpu(t, 257, 0, chunk=100)
    for k in ("ton", "T", "moments"):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    assert run_gpu(t, 257, 0, seed=78)["ton"].tobytes() != a["ton"].tobytes()
    empty = tn.make_table([0], [], [], [], [], [], [], [], params())
    r = tn.simulate(empty, 5, 1)
    assert r["T"].shape == (5, 1) and (r["T"] == 0).all() and r["moments"].shape == (0, 2)


def test_bad_arguments_are_refused_and_nothing_is_launched(lib):
    t = TABLES["four"]
    F, E, P, K = 4, int(t["area"].shape[0]), 3, 8
    dev = {k: torch.from_numpy(t[k]).cuda() for k in ("entry_start", "area", "err", "flags", "depth", "pass_id", "params")}
    ton = torch.full((K * F + 1,), -77.0, dtype=torch.float64, device="cuda")
    T = torch.full((K * P,), -77.0, dtype=torch.float64, device="cuda")
    mom = torch.full((F, 2), -77.0, dtype=torch.float64, device="cuda")
    start_h, pp_h, pr = t["entry_start"].copy(), t["params"].copy(), t["probs"].copy()
    st = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(seed=1, k0=0, K=K, start=dev["entry_start"].data_ptr(), start_h=start_h, F=F, area=dev["area"].data_ptr(), err=dev["err"].data_ptr(),
                 flags=dev["flags"].data_ptr(), E=E, depth=dev["depth"].data_ptr(), pass_id=dev["pass_id"].data_ptr(), pp=dev["params"].data_ptr(),
                 pp_h=pp_h, P=P, mix=t["mix"], m=t["min_depth"], pr=pr, ton=ton.data_ptr())
        a.update(kw)
        host = lambda v: None if v is None else v.ctypes.data
        return lib.aq_tonnage_simulate_f64(a["seed"], a["k0"], a["K"], a["start"], host(a["start_h"]), a["F"], a["area"], a["err"], a["flags"], a["E"],
                                           a["depth"], a["pass_id"], a["pp"], host(a["pp_h"]), a["P"], a["mix"], a["m"], host(a["pr"]), a["ton"], st)

    def changed(arr, i, v):
        b = arr.copy()
        b.reshape(-1)[i] = v
        return b

    bad = [dict(K=1 << 31), dict(F=1 << 31), dict(E=1 << 31), dict(K=-1), dict(k0=-1), dict(k0=(1 << 32) - 7), dict(k0=(1 << 63) - 1), dict(P=0), dict(P=-1),
           dict(mix=-0.1), dict(mix=1.5), dict(mix=float("nan")), dict(m=float("inf")), dict(m=float("nan")),
           dict(start=None), dict(start_h=None), dict(area=None), dict(err=None), dict(flags=None), dict(depth=None), dict(pass_id=None), dict(pp=None),
           dict(pp_h=None), dict(pr=None), dict(ton=None),
           dict(ton=ton.data_ptr() + 4), dict(area=dev["area"].data_ptr() + 4), dict(err=dev["err"].data_ptr() + 8), dict(start=dev["entry_start"].data_ptr() + 2),
           dict(depth=dev["depth"].data_ptr() + 4), dict(pass_id=dev["pass_id"].data_ptr() + 2), dict(pp=dev["params"].data_ptr() + 4),
           dict(pp_h=changed(pp_h, 1, 0.0)), dict(pp_h=changed(pp_h, 7, -1.0)), dict(pp_h=changed(pp_h, 0, np.nan)), dict(pp_h=changed(pp_h, 17, np.inf)),
           dict(pr=changed(pr, 2, np.nan)),
           dict(start_h=changed(start_h, 2, 0)), dict(start_h=changed(start_h, 0, -1)), dict(start_h=changed(start_h, 4, E + 1))]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert lib.aq_last_error().startswith(b"tonnage:"), kw
    red = lambda **kw: lib.aq_tonnage_reduce_f64(*[{**dict(ton=ton.data_ptr(), K=K, F=F, pass_id=dev["pass_id"].data_ptr(), P=P, T=T.data_ptr(),
                                                           mom=mom.data_ptr()), **kw}[k] for k in ("ton", "K", "F", "pass_id", "P", "T", "mom")], st)
    for kw in (dict(K=1 << 31), dict(F=1 << 31), dict(P=-1), dict(ton=None), dict(pass_id=None), dict(T=None), dict(mom=None), dict(mom=mom.data_ptr() + 8),
               dict(T=T.data_ptr() + 4), dict(ton=ton.data_ptr() + 4)):
        assert red(**kw) != 0, kw
    c4 = torch.zeros((3, 4), dtype=torch.int32, device="cuda")
    out = torch.full((3,), -77.0, dtype=torch.float64, device="cuda")
    assert lib.aq_tonnage_uniform_f64(1, None, 3, out.data_ptr(), st) != 0 and lib.aq_tonnage_uniform_f64(1, c4.data_ptr(), 3, out.data_ptr() + 4, st) != 0
    assert lib.aq_tonnage_ndtri_f64(out.data_ptr(), 3, None, st) != 0 and lib.aq_tonnage_ndtri_f64(out.data_ptr() + 4, 3, out.data_ptr(), st) != 0
    assert call(F=0) == 0 and call(K=0) == 0 and red(K=0) == 0      # nothing to do: nothing written
    torch.cuda.synchronize()
    assert bool((ton == -77.0).all()) and bool((T == -77.0).all()) and bool((mom == -77.0).all()) and bool((out == -77.0).all())
    assert call() == 0                                      # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert np.array_equal(bits(ton[:K * F].cpu().numpy().reshape(K, F)), bits(tn.simulate_numpy(t, K, 1, 0))) and float(ton[K * F]) == -77.0


# ---- the command lines ----

def test_command_line_writes_the_cpu_runs_bytes(lib, tmp_path):
    labels, csv_path = synthetic_run(tmp_path)
    factors = write(tmp_path / "factors.csv", "pass,s_mean,s_sd,h_mean,h_sd\n2013-2015,12,3,0.8,0.1\n")
    errors = write(tmp_path / "errors.csv", "pass,farm_type,model_error_mean,model_error_sd\n2013-2015,circle_farm,0.1,2\n2013-2015,square_farm,-0.2,3\n")
    depths = write(tmp_path / "depths.csv", "facility_index,cage_depth\n1,7.5\n")
    files = []
    for extra in ((), ("--cpu",)):
        out = tmp_path / ("cpu" if extra else "gpu")
        r = subprocess.run([sys.executable, "-m", "aquaculture_amd.tonnage", "--labels", labels, "--geocode-bboxes", csv_path, "--tonnage-factors", factors,
                            "--tonnage-errors", errors, "--tonnage-depths", depths, "--tonnage-K", "500", "--tonnage-seed", "3", "--out", str(out), *extra],
                           cwd=ROOT, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "2 facilities, 1 passes, K = 500" in r.stdout, r.stdout
        files.append({f: open(out / f, "rb").read() for f in (tn.ESTIMATES_FILE, tn.FACILITIES_FILE)})
        assert json.load(open(out / tn.JSON_FILE))["cpu"] is bool(extra)
    assert files[0] == files[1]
    assert len(files[0][tn.FACILITIES_FILE].decode().splitlines()) == 3


def test_detect_py_writes_the_tonnage_of_its_own_sweep(lib, tmp_path):
    """The tiny sweep of tests/test_gpu_facilities.py's last test with --tonnage: the three files, equal to what the restatement makes of
    the run's label files; --facilities-by year leaves the facility file per year while the tonnage groups by pass."""
    from PIL import Image
    from aquaculture_amd import checkpoint, geocode, tiles
    (tmp_path / "jpegs").mkdir()
    for k, i in enumerate((0, 3, 19, 20)):
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * k}_0.jpeg", quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    factors = write(tmp_path / "factors.csv", "pass,s_mean,s_sd,h_mean,h_sd\n2013-2015,12,3,0.8,0.1\n")
    args = ["--facilities-conf", "0.25", "--facilities-eps", "25", "--facilities-min-cages", "4", "--facilities-by", "year", "--facilities"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"), "--source",
                        str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "ton",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, *args, "--tonnage", "--tonnage-factors", factors, "--tonnage-K", "200"],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "ton"
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path)
    want = tn.tonnage_from_table(table, str(tmp_path / "want"), factors, K=200, conf_thresh=0.25, eps=25.0, min_cages=4, widths=640, heights=640, cpu=True)
    assert f"tonnage: {tn.describe(want)}" in r.stdout + r.stderr
    for f in (tn.ESTIMATES_FILE, tn.FACILITIES_FILE):
        assert open(run / f, "rb").read() == open(tmp_path / "want" / f, "rb").read(), f
    doc = json.load(open(run / tn.JSON_FILE))
    assert doc["K"] == 200 and doc["cpu"] is False and doc["device"] != "cpu"
    print(tn.describe(want))
    assert len(want["facility_index"]) >= 1 and sum(want["facility_cages"]) >= 4 and all(v > 0 for v in want["tonnage"])     # real numbers, not headers
    assert "year" in json.load(open(run / "facilities.geojson"))["features"][0]["properties"]
    assert "tonnage" not in json.load(open(run / "run_params.json"))
