"""`voxelPS --render-keyframes` on the sokrates fixture (tests/golden/sokrates_small): the re-rendered keyframes decode at the keyframe size,
render_report.txt has one row per keyframe, and every file a run without the flag writes is byte-identical to the same file of the run with it."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "psgradientsdf_amd", "host", "voxelPS")
GOLD = os.path.join(ROOT, "tests", "golden", "sokrates_small")


def _run(out, extra):
    os.makedirs(out)
    cfg = {"input": GOLD + "/", "output": out, "pose filename": "pose.txt", "datatype": "multiview", "first": 0, "last": 7, "voxel size": 0.004,
           "truncation factor": 5, "zmin": 0.5, "zmax": 3.5, "sharpness threshold": 0.0, "model type": "SH1", "loss function": "cauchy",
           "reg albedo": 0.0, "reg norm": 10.0, "reg laplacian": 0.0, "max iter": 6, "damping": 1.0, "converge threshold": 1e-9, "lambda": 0.2,
           "upsample": False, "--light": True, "--albedo": True, "--distance": True, "--pose": True}
    json.dump(cfg, open(out + "config.json", "w"))
    r = subprocess.run([EXE, "--config_file", out + "config.json"] + extra, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def _files(d):
    return sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)


def test_render_keyframes_on_sokrates(built, tmp_path):
    from PIL import Image
    a, b = str(tmp_path / "plain") + "/", str(tmp_path / "render") + "/"
    _run(a, [])
    _run(b, ["--render-keyframes"])
    plain, rendered = _files(a), _files(b)
    extra = [f for f in rendered if f not in plain]
    assert set(plain) <= set(rendered)
    for f in plain:
        if f == "config.json" or f == "saved_config.json":
            continue                                                    # (they name the output directory)
        assert open(a + f, "rb").read() == open(b + f, "rb").read(), f
    rows = [l.split() for l in open(b + "render_report.txt") if not l.startswith("#")]
    W, H = Image.open(os.path.join(GOLD, "color000001.png")).size
    assert len(rows) >= 2 and all(len(r) == 6 for r in rows)
    pngs = [f for f in extra if f.endswith(".png")]
    assert len(pngs) == 4 * len(rows) and "render_report.txt" in extra
    for name, hits, _, rmse, psnr, robust in rows:
        assert int(hits) > 1000 and 0 < float(rmse) < 0.2 and float(psnr) > 10
        for kind in ("rendered", "albedo", "shading", "residual"):
            im = Image.open(os.path.join(b, "render", f"{name}_{kind}.png"))
            assert im.size == (W, H)
            assert np.asarray(im).max() > 0
    print("sokrates re-rendering after the run:", [(r[0], r[3], r[4]) for r in rows])
