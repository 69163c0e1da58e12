"""CPU-side checks of the drop-in boundary: the HIP library builds for gfx950, loads without a GPU and
exports every symbol include/psgsdf.h declares; argument errors come back as status codes."""
import ctypes

import pytest

from psgradientsdf_amd import capi


def test_engine_exports_every_declared_symbol(built):
    import __graft_entry__ as g
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    names = g._declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), n
    lib.psgsdf_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.psgsdf_version()


def test_oracle_mirrors_the_abi(built):
    import __graft_entry__ as g
    from oracle import oracle
    lib = oracle.lib()
    # (the oracle's multi-rank mirror is driven through its own phase API by tests/_slab_runner.py: no communicator entry points)
    skip = {"psgsdf_comm_unique_id", "psgsdf_comm_init_ext", "psgsdf_comm_init_sockets", "psgsdf_comm_allreduce_host", "psgsdf_comm_stats", "psgsdf_kernel_times", "psgsdf_reset_kernel_times",
            "psgsdf_set_profiling", "psgsdf_watch_kernel", "psgsdf_debug_time_pcg_pass", "psgsdf_debug_time_pcg_solve", "psgsdf_debug_rare_rows", "psgsdf_debug_sync_stats", "psgsdf_debug_normals_cache", "psgsdf_debug_overlap_probe", "psgsdf_set_keyframes_frames",
            "psgsdf_slab_plane_count", "psgsdf_plan_slab", "psgsdf_upload_volume_slab", "psgsdf_rebalance_slabs", "psgsdf_set_record_observer", "psgsdf_set_on_iter_period", "psgsdf_get_tuning",
            "psgsdf_extract_mesh", "psgsdf_extract_pointcloud", "psgsdf_extract_sdf"}      # (the writers' geometry on the device: the oracle's counterpart is the host-side pass of psgradientsdf_amd/host)
    for n in g._declared_symbols():
        if n in skip:
            continue
        assert hasattr(lib, n.replace("psgsdf_", "orc_")), n


def test_dangerous_knobs_are_not_in_the_product_library(built):
    """the fault-injection / ablation / "skip the check words" environment variables are compiled into libpsgsdf_dev.so only; the
    product library does not even contain their names as knobs it honours (they appear once, in the list of variables it reports as IGNORED)."""
    import os
    prod = open(capi.ENGINE_LIB, "rb").read(); dev = open(capi.ENGINE_LIB_DEV, "rb").read()
    lib = ctypes.CDLL(capi.ENGINE_LIB); lib.psgsdf_version.restype = ctypes.c_char_p
    devlib = ctypes.CDLL(capi.ENGINE_LIB_DEV); devlib.psgsdf_version.restype = ctypes.c_char_p
    assert b"dev" not in lib.psgsdf_version() and b"dev" in devlib.psgsdf_version()
    for n in g_names():
        assert hasattr(devlib, n), n
    for k in (b"PSGSDF_FAULT_SOLVE", b"PSGSDF_FAULT_HALO", b"PSGSDF_PCG_ABLATE", b"PSGSDF_MBOX_CHECK"):
        assert prod.count(k) == 1 and dev.count(k) >= 1, k      # (one occurrence: the kDevKnobs name table behind "ignored_dev_only")
    for k in (b"PSGSDF_PCG_PIPELINE", b"PSGSDF_PCG_FUSE_ASM", b"PSGSDF_PCG_TAGM", b"PSGSDF_PCG_XCD_LOCAL", b"PSGSDF_PCG_PREFETCH"):
        assert k not in prod and k not in dev, k      # (retired with the persistent kernels and the slower paths they selected: no build knows them)
    assert os.path.getsize(capi.ENGINE_LIB_DEV) > 0


def g_names():
    import __graft_entry__ as g
    return g._declared_symbols()


def test_comm_entry_points_fail_cleanly_without_a_gpu(built):
    """the communicator entry points are status codes too: no context -> ARG; a NULL id -> ARG; librccl is only bound when asked for"""
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    for f in ("psgsdf_comm_init", "psgsdf_comm_init_ext", "psgsdf_comm_unique_id", "psgsdf_comm_stats"):
        getattr(lib, f).restype = ctypes.c_int
    assert lib.psgsdf_comm_init(None, None, 0, 1) == -1
    assert lib.psgsdf_comm_init_ext(None, None, 0, 1) == -1
    assert lib.psgsdf_comm_unique_id(None) == -1
    assert lib.psgsdf_comm_stats(None, None) == -1
    import subprocess, sys
    code = ("import ctypes; lib = ctypes.CDLL(%r); lib.psgsdf_comm_init(None, None, 0, 1); "
            "print('librccl' in open('/proc/self/maps').read())" % capi.ENGINE_LIB)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert out.stdout.strip() == "False", out.stdout + out.stderr      # loading the engine pulls no RCCL into a single-GPU process


def test_bad_arguments_are_status_codes(built):
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    lib.psgsdf_create.restype = ctypes.c_int
    assert lib.psgsdf_create(None, None, None, 0, None) == -1
    st = capi.default_settings(capi.SH1); st.model = 7
    g = capi.GridDesc(); g.dim[:] = [8, 8, 8]; g.voxel_size = 0.01
    K = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    ctx = ctypes.c_void_p()
    assert lib.psgsdf_create(ctypes.byref(g), K, ctypes.byref(st), 0, ctypes.byref(ctx)) == -1   # unknown model


def test_no_cpu_fallback_without_library(monkeypatch, tmp_path):
    monkeypatch.setattr(capi, "ENGINE_LIB", str(tmp_path / "missing.so"))
    monkeypatch.setattr(capi, "_engine_lib", {})
    with pytest.raises(capi.PsgsdfError):
        capi.engine_lib()


def test_everything_compiles_from_scratch_in_a_clean_copy(tmp_path):
    """VERDICT r03 housekeeping: the objects, the library and the host binaries travel with the snapshot, so a green suite does not show that the tree
    BUILDS.  Copy the sources only (no .o / .so / binaries) to a scratch directory, run the Makefiles there (hipcc --offload-arch=gfx950 cross-compiles
    without a GPU; ~25 s on 16 jobs), and check the fresh library against the header and the fresh oracle against its loader."""
    import os, re, shutil, subprocess, time
    import __graft_entry__ as g
    root = g.ROOT
    keep = re.compile(r"\.(hip|h|hpp|cpp|c|inc|py)$|^Makefile$")
    for sub in ("psgradientsdf_amd/csrc", "psgradientsdf_amd/host", "include", "oracle"):
        dst = tmp_path / sub
        dst.mkdir(parents=True)
        for f in os.listdir(os.path.join(root, sub)):
            if keep.search(f) and os.path.isfile(os.path.join(root, sub, f)):
                shutil.copy(os.path.join(root, sub, f), dst / f)
    assert not list(tmp_path.rglob("*.o")) and not list(tmp_path.rglob("*.so"))
    t0 = time.time()
    subprocess.run(["make", "-s", "-j16", "-C", str(tmp_path / "psgradientsdf_amd/csrc")], check=True, timeout=1500)
    subprocess.run(["make", "-s", "-C", str(tmp_path / "oracle")], check=True, timeout=600)
    print(f"from scratch: {time.time() - t0:.0f} s")
    lib = ctypes.CDLL(str(tmp_path / "psgradientsdf_amd/csrc/libpsgsdf.so"))
    for n in g._declared_symbols():
        assert hasattr(lib, n), n
    lib.psgsdf_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.psgsdf_version()
    for exe in ("voxelPS", "voxelps_scene"):
        assert os.access(tmp_path / "psgradientsdf_amd/host" / exe, os.X_OK), exe
    olib = ctypes.CDLL(str(next((tmp_path / "oracle").glob("*.so"))))
    assert hasattr(olib, "orc_iterate")
    # the strict-arithmetic development variant (device_common.h PSG_STRICT, tools/deviations.py) must keep compiling too: every deviation switched off
    t0 = time.time()
    subprocess.run(["make", "-s", "-j16", "-C", str(tmp_path / "psgradientsdf_amd/csrc"), "strict", "STRICT=31"], check=True, timeout=1500)
    print(f"strict variant: {time.time() - t0:.0f} s")
    slib = ctypes.CDLL(str(tmp_path / "psgradientsdf_amd/csrc/libpsgsdf_strict31.so"))
    assert hasattr(slib, "psgsdf_set_frame_solver") and b"dev" in ctypes.cast(slib.psgsdf_version, ctypes.CFUNCTYPE(ctypes.c_char_p))()
