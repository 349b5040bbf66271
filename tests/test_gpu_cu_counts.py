"""No result may depend on the CU count a persistent grid is sized for.

More than twenty launchers size their grid as min(aq_cus() * k, n_tiles) and let every workgroup walk tile, tile + G, tile + 2 G, ...;
aq_cus() is the device's CU count or AQ_NUM_CUS, read once per process.  On a whole MI355X every small test shape has fewer tiles than
workgroups, so the loops' second trip, their double buffers' second phase and their last-trip paths never run in the rest of the suite.
Here the case list of tests/cu_cases.py (every such launcher at its smallest hard shapes, a tile ladder of 1 .. 25 tiles per convolution
family in whole tiles, with a partial last tile and, for the families tiled in image rows, with a partial tile in the middle of the walk,
the image-side launchers, the whole engine) runs once per value of AQ_NUM_CUS in {unset, 1, 2, 3,
13}, each in a fresh child process, one after another.  At 1, 2 and 3 CUs the ladders give workgroups of 1, 2, 3 and >= 4 trips with uneven
last trips; 13 is odd and above 8, so the XCD-aware first_tile map runs with G & 7 != 0 and G >> 3 >= 1.

Per child: it exits 0; every case meets its family's own reference and tolerance (the unset child too, so the shapes are not vacuous);
the case ids are the committed list's; and every case's sha256 over its owned output bytes equals the unset child's -- no tolerance:
which workgroup computes a tile must not change a byte.  The only exemptions are the ids of cu_cases.EXEMPT (the head-decode candidate
lists, whose row order follows atomic counters: their digest is taken over the rows sorted by candidate index).  The engine cases also
record last_launches() and the detections themselves, which must not change either.  Cases that launch nothing (a refused halo
configuration, an assembly family the build does not hold) are marked `skipped` by the child, listed here and must be of those two kinds.

AQ_NUM_CUS is never set above the device's own CU count: grids larger than the chip are not a configuration the persistent kernels
support.

Measured on MI355X (wall time of a child, import to exit; 1382 cases, of which 73 launch nothing in a default build: 63 of the
experimental planar assembly families, 10 refused halo configurations), two runs: unset 8.9 and 9.6 s, 1: 9.4 and 10.4 s, 2: 9.7 and
9.8 s, 3: 9.5 and 9.5 s, 13: 9.9 and 9.6 s (the second run of each pair with 17 cases fewer), of which about 7 s are the cases themselves
(host-side references included).  LIMIT is three times the slowest, rounded up to ten seconds.
"""
import json
import os
import subprocess
import sys
import time

import pytest

import cu_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = [None, 1, 2, 3, 13]
LIMIT = "40"                     # seconds: 3 x the slowest child's 10.4 s (over both measured runs), rounded up to ten seconds
FAULT_STATUS = (124, 137, 134, 139, -6, -9, -11, 3)        # 3: the child's own status after a HIP error (cu_cases.main)

_children = {}                   # AQ_NUM_CUS value -> (exit status, records by id, output, seconds)
_faulted = []                    # the value whose child faulted: nothing more is started after it


def child(value, tmp_path_factory):
    """The records of the child run with AQ_NUM_CUS = value (None: unset), started at most once."""
    if value in _children:
        return _children[value]
    if _faulted:
        pytest.fail(f"not run: an earlier child faulted (AQ_NUM_CUS={_faulted[0]})")
    out = tmp_path_factory.mktemp("cu") / f"cases_{value}.json"
    env = {k: v for k, v in os.environ.items() if k != "AQ_NUM_CUS"}
    if value is not None:
        env["AQ_NUM_CUS"] = str(value)
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", LIMIT, sys.executable, os.path.join("tests", "cu_cases.py"), "--out", str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    seconds = time.perf_counter() - t0
    text = r.stdout[-2000:] + r.stderr[-4000:]
    print(f"AQ_NUM_CUS={value}: child exit {r.returncode} after {seconds:.1f} s")
    if r.returncode in FAULT_STATUS or "illegal memory access" in text:
        _faulted.append(value)
    records = {}
    if out.exists():
        data = json.loads(out.read_text())
        assert data["num_cus_env"] == (None if value is None else str(value))
        records = {rec["id"]: rec for rec in data["cases"]}
    _children[value] = (r.returncode, records, text, seconds)
    return _children[value]


@pytest.mark.parametrize("value", VALUES, ids=["unset" if v is None else str(v) for v in VALUES])
def test_results_do_not_depend_on_the_cu_count(lib, tmp_path_factory, value):
    if _faulted and value not in _children:                  # before anything here opens the GPU
        pytest.fail(f"not run: an earlier child faulted (AQ_NUM_CUS={_faulted[0]})")
    if value is not None:
        import torch
        assert value <= torch.cuda.get_device_properties(0).multi_processor_count, "AQ_NUM_CUS above the device's CU count is not supported"
    base_rc, base, base_text, _ = child(None, tmp_path_factory)
    assert base_rc == 0 and base, f"the unset child exited {base_rc}:\n{base_text}"
    rc, records, text, _ = child(value, tmp_path_factory)
    assert rc == 0, f"AQ_NUM_CUS={value}: child exited {rc}:\n{text}"
    bad = [(i, r.get("error")) for i, r in records.items() if not r["ok"]]
    assert not bad, f"AQ_NUM_CUS={value}: {len(bad)} cases miss their reference, first {bad[:5]}"
    committed = {c.id: c for c in cu_cases.CASES}
    assert set(records) == set(base) == set(committed), sorted(set(records) ^ set(committed))[:10]
    for i, r in records.items():
        assert r["n_tiles"] == committed[i].n_tiles, i
    # cases that launched nothing: only what the launchers refuse by the layer's shape and what this build does not hold, the same in every child
    skipped = sorted(i for i, r in records.items() if r.get("skipped"))
    print(f"AQ_NUM_CUS={value}: {len(skipped)} of {len(records)} cases launched nothing: "
          f"{sorted({records[i]['skipped'].split(':')[0] + ' ' + i.rsplit('-', 2)[0] for i in skipped})}")
    assert skipped == sorted(i for i, r in base.items() if r.get("skipped"))
    for i in skipped:
        halo = committed[i].family == "conv2d" and committed[i].geom[1] >= len(cu_cases.IGEMM_TILES) and records[i]["skipped"].startswith("refused")
        experimental = any(f"conv3x3_pl-{b}-" in i for b in cu_cases.EXPERIMENTAL_BUILDS) and records[i]["skipped"].startswith("not built")
        assert halo or experimental, (i, records[i]["skipped"])
    launched = set(records) - set(skipped)
    assert {c.family for c in cu_cases.CASES if c.id in launched} >= {c.family for c in cu_cases.CASES} - {f"conv3x3_pl-{b}" for b in cu_cases.EXPERIMENTAL_BUILDS}
    differing = [i for i, r in records.items() if r["sha256"] != base[i]["sha256"]]
    assert not differing, (f"AQ_NUM_CUS={value}: the owned output bytes of {len(differing)} cases differ from the unset child's, first "
                           f"{[(i, records[i]['n_tiles']) for i in differing[:8]]}")
    engines = [i for i in records if i.startswith("engine-")]
    assert len(engines) == 5
    for i in engines:
        assert records[i]["last_launches"] and records[i]["last_launches"] == base[i]["last_launches"], i
        assert records[i]["boxes"] == base[i]["boxes"] > 100, i
        assert records[i]["counts"] == base[i]["counts"] and records[i]["detections"] == base[i]["detections"], i       # bit for bit: float32 in doubles
