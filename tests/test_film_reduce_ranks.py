"""hk_film_reduce with 2 and 3 ranks (include/hikari_mi355x.h, the "Multi-GPU behind the C-ABI" block of hk_comm.cpp).

Real RCCL puts one rank per device and the test box has one GPU, so the ranks here talk through a test double of librccl.so.1
(tests/native/fake_rccl.cpp): host-only, built into a directory of the test's own, found first by the library's dlopen because the
workers' LD_LIBRARY_PATH starts with that directory.  The double's ncclReduce is asynchronous and stream-ordered like the real one
(device -> pinned copy, a host function that sums in rank order on the root, pinned -> device copy on the root), so what is tested is
the library's side of the exchange: the flush of noted calls and the join of the pipeline lanes before the reduce, count, dtype and
root, the untouched non-root film, work after the reduce, error returns.  Every rank is a fresh `python tests/film_reduce_worker.py`
that never imports torch; the workers of one world size run all their scenarios in one start-up and save .npy files that the tests
below compare with the rank-order sum of each rank's own reference film (rendering is deterministic) and with the whole frame."""
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLE_SRC = os.path.join(ROOT, "tests", "native", "fake_rccl.cpp")
WORKER = os.path.join(ROOT, "tests", "film_reduce_worker.py")
HK_COMM_SRC = os.path.join(ROOT, "hikari.jl_amd", "csrc", "hk_comm.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
W, H = 67, 45                   # tests/film_reduce_worker.py
COUNT = 4 * W * H               # [rgb 3N | weight N]
HK_ERR_DEVICE, HK_ERR_UNSUPPORTED = -2, -3
WORKER_TIMEOUT = 600            # seconds for one set of workers (all their scenarios)


def build_double(out_dir, *defines):
    """-> (returncode, compiler output); the library is out_dir/librccl.so.1"""
    os.makedirs(out_dir, exist_ok=True)
    cmd = [HIPCC, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-Wl,-soname,librccl.so.1", *defines, DOUBLE_SRC,
           "-o", os.path.join(out_dir, "librccl.so.1")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout + r.stderr


@pytest.fixture(scope="module")
def double_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fake_rccl"))
    rc, out = build_double(d)
    assert rc == 0, out
    return d


def worker_env(double_dir, run_dir, **extra):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = double_dir + (":" + env["LD_LIBRARY_PATH"] if env.get("LD_LIBRARY_PATH") else "")
    env["FAKE_RCCL_DIR"] = run_dir
    env.pop("FAKE_RCCL_FAIL", None)
    env.update(extra)
    return env


def read_log(run_dir):
    path = os.path.join(run_dir, "fake_rccl.log")
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [(line.split()[0], dict(t.split("=", 1) for t in line.split()[1:] if "=" in t)) for line in f if line.strip()]


# ---------------------------------------------------------------------------------------------------------------- CPU: the double
def test_double_builds_warning_free(tmp_path):
    rc, out = build_double(str(tmp_path / "plain"))
    assert rc == 0, out
    rc, out = build_double(str(tmp_path / "no_group_end"), "-DFAKE_RCCL_OMIT_GROUP_END")
    assert rc == 0, out


def test_double_exports_exactly_what_the_library_resolves(double_dir):
    with open(HK_COMM_SRC) as f:
        wanted = set(re.findall(r'\bsym\("(\w+)"\)', f.read()))
    assert len(wanted) == 8, wanted
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(double_dir, "librccl.so.1")], capture_output=True, text=True, check=True)
    exported = {parts[2] for parts in (line.split() for line in r.stdout.splitlines()) if len(parts) == 3 and parts[1] == "T"}
    assert exported == wanted


PROBE = r'''
import ctypes as C, os, sys
sys.path[:0] = [%(root)r]
import hikari_jl_amd as hk
L = hk._lib.lib()
buf = (C.c_uint8 * 128)()
rc = L.hk_comm_unique_id(buf)
maps = sorted({l.split()[-1] for l in open("/proc/self/maps") if "librccl" in l.split()[-1]})
assert "torch" not in sys.modules
print(rc)
print(bytes(buf)[:8].decode("latin-1"))
print(bytes(buf)[16:].split(b"\0")[0].decode("latin-1"))
print((L.hk_last_error() or b"").decode())
print(":".join(maps))
'''


def probe_unique_id(double_dir, run_dir):
    r = subprocess.run([sys.executable, "-c", PROBE % {"root": ROOT}], env=worker_env(double_dir, run_dir), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rc, magic, name, err, maps = (r.stdout.splitlines() + [""] * 5)[:5]
    return int(rc), magic, name, err, [m for m in maps.split(":") if m]


def test_unique_id_comes_from_the_double(double_dir, tmp_path):
    """no device needed: hk_comm_unique_id loads librccl from the double's directory (RUNPATH, not RPATH) and returns its magic; the
    id names a shared file the double created in FAKE_RCCL_DIR.  The directory is deliberately longer than the 128-byte id: the id
    carries the file's name only."""
    run_dir = tmp_path / ("d" * 70) / ("e" * 70)
    run_dir.mkdir(parents=True)
    assert len(str(run_dir)) > 128
    rc, magic, name, err, maps = probe_unique_id(double_dir, str(run_dir))
    assert rc == 0, err
    assert magic == "FAKERCCL"
    assert maps and all(os.path.dirname(m) == double_dir for m in maps), maps
    assert name.endswith(".shm") and "/" not in name
    assert sorted(os.listdir(run_dir)) == sorted([name, "fake_rccl.log"])
    assert [e[0] for e in read_log(str(run_dir))] == ["ncclGetUniqueId"]


def test_librccl_without_group_end_is_unsupported(tmp_path):
    d = str(tmp_path / "lib")
    rc, out = build_double(d, "-DFAKE_RCCL_OMIT_GROUP_END")
    assert rc == 0, out
    rc, magic, name, err, maps = probe_unique_id(d, str(tmp_path))
    assert rc == HK_ERR_UNSUPPORTED
    assert "librccl lacks ncclGroupEnd" in err
    assert maps and all(os.path.dirname(m) == d for m in maps), maps


# ------------------------------------------------------------------------------------------------------------- GPU: the workers
def run_workers(double_dir, run_dir, world, scenarios, initrank_failure=False, local=False, **env_extra):
    """world fresh processes (all on cuda:0) run `scenarios`; -> per-rank result dicts.  Any failure or timeout kills every rank and
    fails the test: nothing is retried."""
    os.makedirs(run_dir, exist_ok=True)
    spec = {"world": world, "dir": run_dir, "double_dir": double_dir, "scenarios": scenarios, "initrank_failure": initrank_failure,
            "local": local}
    spec_path = os.path.join(run_dir, "spec.json")
    with open(spec_path, "w") as f:
        json.dump(spec, f)
    env = worker_env(double_dir, run_dir, **env_extra)
    logs = [open(os.path.join(run_dir, "worker_r%d.txt" % r), "w") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, spec_path, str(r)], env=env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(world)]
    deadline = time.monotonic() + WORKER_TIMEOUT
    timed_out = False
    try:
        for p in procs:
            p.communicate(timeout=max(1.0, deadline - time.monotonic()))
            if p.returncode != 0:
                break                      # one rank failed: the others would only wait for it
    except subprocess.TimeoutExpired:
        timed_out = True
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
        for f in logs:
            f.close()

    def tail(r):
        with open(os.path.join(run_dir, "worker_r%d.txt" % r)) as f:
            return f.read()[-3000:]
    assert not timed_out, "workers timed out:\n" + "\n".join(tail(r) for r in range(world))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d exited with %s:\n%s" % (r, p.returncode, tail(r))
    results = []
    for r in range(world):
        with open(os.path.join(run_dir, "result_r%d.json" % r)) as f:
            results.append(json.load(f))
    for res in results:
        assert res["torch_imported"] is False
        assert res["librccl_maps"] and all(os.path.dirname(m) == double_dir for m in res["librccl_maps"])
        assert res["unique_id_magic"] == "FAKERCCL"
    return results


class Run:
    def __init__(self, run_dir, world, results):
        self.dir, self.world, self.results = run_dir, world, results

    def arr(self, scenario, rank, name):
        return np.load(os.path.join(self.dir, "%s_r%d_%s.npy" % (scenario, rank, name)))

    def rank_order_sum(self, scenario):
        total = self.arr(scenario, 0, "ref").copy()
        for r in range(1, self.world):
            total = total + self.arr(scenario, r, "ref")   # in the element type, rank order: what the double's root computes
        return total

    def reduces(self, scenario, rank):
        return self.results[rank]["scenarios"][scenario]["reduces"]

    def check_log(self, scenario, root, dtype, frames=1):
        for r in range(self.world):
            calls = self.reduces(scenario, r)
            assert len(calls) == frames, (scenario, r, calls)
            for c in calls:
                assert (int(c["rank"]), int(c["count"]), int(c["dtype"]), int(c["root"]), int(c["group"])) == (r, COUNT, dtype, root, 0), c

    def check_reduced(self, scenario, root, exact_whole=False):
        """root: the rank-order sum of the reference films bit for bit, and the whole frame (to rounding: the sum runs in another order);
        every other rank: its own reference film, untouched"""
        expect = self.rank_order_sum(scenario)
        out = self.arr(scenario, root, "out")
        assert np.isfinite(out).all()
        assert np.array_equal(out, expect)
        whole = self.arr(scenario, root, "whole")
        if exact_whole:
            assert np.array_equal(out, whole)
        else:
            assert np.allclose(out, whole, rtol=1e-5, atol=1e-6)
        assert (out[3 * W * H:] > 0).all()                     # every pixel has samples of every rank
        for r in range(self.world):
            if r != root:
                assert np.array_equal(self.arr(scenario, r, "out"), self.arr(scenario, r, "ref")), (scenario, r)


LANES = {"HK_BATCH_PATHS_M": "0", "HK_PIPELINE": "4", "HK_PIPELINE_AFTER": "0"}   # every call at once, each on the next lane
WORLD2 = [
    {"name": "a", "root": 0, "samples": 8},
    {"name": "c", "root": 0, "samples": 8, "f64": True},
    {"name": "d_batched", "root": 0, "samples": 12, "one_sample_calls": True},
    {"name": "d_lanes", "root": 0, "samples": 12, "one_sample_calls": True, "knobs": LANES},
    {"name": "e_batched", "root": 0, "samples": 8, "filter": "box", "one_sample_calls": True, "extra_samples": 3},
    {"name": "e_lanes", "root": 0, "samples": 8, "filter": "box", "one_sample_calls": True, "extra_samples": 3, "knobs": LANES},
    {"name": "f", "root": 1, "samples": 8, "scene": "integration", "tiles": True},
    {"name": "g", "root": 0, "samples": 8, "frames": 3},
]
WORLD3 = [
    {"name": "b", "root": 1, "samples": 8},
    {"name": "b_f64", "root": 2, "samples": 8, "f64": True},
    {"name": "f", "root": 2, "samples": 8, "scene": "integration", "tiles": True},
]


@pytest.fixture(scope="module")
def world2(double_dir, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("world2"))
    return Run(d, 2, run_workers(double_dir, d, 2, WORLD2))


@pytest.fixture(scope="module")
def world3(double_dir, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("world3"))
    return Run(d, 3, run_workers(double_dir, d, 3, WORLD3))


@pytest.mark.gpu
def test_a_sample_sharding_two_ranks(world2):
    world2.check_reduced("a", root=0)
    world2.check_log("a", root=0, dtype=7)
    # the whole run: one ncclReduce per rank per frame, never inside a group (one film per process), no group calls at all
    log = read_log(world2.dir)
    for r in range(2):
        n = sum(len(world2.reduces(sc["name"], r)) for sc in WORLD2)
        assert n == sum(sc.get("frames", 1) for sc in WORLD2)
        assert sum(1 for name, f in log if name == "ncclReduce" and f["rank"] == str(r)) == n
    assert not [e for e in log if e[0] in ("ncclGroupStart", "ncclGroupEnd") or e[0].startswith("ERROR")], log


@pytest.mark.gpu
def test_b_three_ranks_root_one(world3):
    world3.check_reduced("b", root=1)
    world3.check_log("b", root=1, dtype=7)
    world3.check_reduced("b_f64", root=2)
    world3.check_log("b_f64", root=2, dtype=8)
    assert not [e for e in read_log(world3.dir) if e[0].startswith("ERROR")]


@pytest.mark.gpu
def test_c_float64_film(world2):
    assert world2.arr("c", 0, "out").dtype == np.float64
    world2.check_reduced("c", root=0)
    world2.check_log("c", root=0, dtype=8)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["batched", "lanes"])
def test_d_one_sample_calls_are_flushed_before_the_reduce(world2, mode):
    """each rank's share as one-sample calls: batched into a note (the default) or rendered at once on the pipeline lanes — either way
    hk_film_reduce must render the note and join the lanes before its device -> host copy"""
    world2.check_reduced("d_" + mode, root=0)
    world2.check_log("d_" + mode, root=0, dtype=7)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["batched", "lanes"])
def test_e_work_after_the_reduce_is_ordered_behind_it(world2, mode):
    """more one-sample calls on the root right after the reduce, no sync: they must add to the reduced film, not to the film before the
    reduce's host -> device copy lands.  With a box filter every sample adds a weight of exactly 1, so the weights compare exactly."""
    sc = "e_" + mode
    world2.check_log(sc, root=0, dtype=7)
    n = W * H
    for r in range(2):
        share = len(range(r, 8, 2))
        assert (world2.arr(sc, r, "ref")[3 * n:] == share).all()            # one sample adds a weight of exactly 1
    extra = world2.arr(sc, 0, "extra")
    assert (extra[3 * n:] == 3).all()
    reduced = world2.rank_order_sum(sc)
    out = world2.arr(sc, 0, "out")
    assert np.array_equal(out[3 * n:], reduced[3 * n:] + extra[3 * n:])
    assert np.allclose(out[:3 * n], reduced[:3 * n] + extra[:3 * n], rtol=1e-5, atol=1e-6)
    assert np.array_equal(world2.arr(sc, 1, "out"), world2.arr(sc, 1, "ref"))


@pytest.mark.gpu
def test_f_tile_sharding_with_a_medium(world2, world3):
    """pixel bands, one contributor per pixel: x + 0 = x, so the reduced film IS the whole frame, bit for bit"""
    for run, root in ((world2, 1), (world3, 2)):
        run.check_reduced("f", root=root, exact_whole=True)
        run.check_log("f", root=root, dtype=7)


@pytest.mark.gpu
def test_g_three_frames_without_sync(world2):
    world2.check_reduced("g", root=0)
    world2.check_log("g", root=0, dtype=7, frames=3)


@pytest.mark.gpu
def test_h_injected_failures(double_dir, tmp_path):
    """FAKE_RCCL_FAIL=reduce:2: the 2nd hk_film_reduce of every rank returns HK_ERR_DEVICE with the double's message, and the 3rd on the
    same communicator is right.  FAKE_RCCL_FAIL=initrank: hk_comm_create_rank returns HK_ERR_DEVICE and leaves no communicator."""
    scen = [{"name": "h", "root": 0, "samples": 8, "inject": "reduce"}]
    run = Run(str(tmp_path), 2, run_workers(double_dir, str(tmp_path), 2, scen, initrank_failure=True, FAKE_RCCL_FAIL="reduce:2"))
    for r in range(2):
        res = run.results[r]
        h = res["scenarios"]["h"]
        assert h["codes"] == [0, HK_ERR_DEVICE, 0], h
        assert "ncclReduce" in h["messages"][1] and "fake rccl: injected failure" in h["messages"][1], h
        ir = res["initrank"]
        assert ir["code"] == HK_ERR_DEVICE and "fake rccl: injected failure" in ir["message"], ir
        assert ir["out_is_null"] and ir["destroy_null"] == 0, ir
    out = run.arr("h", 0, "out")
    assert np.array_equal(out, run.rank_order_sum("h"))
    assert np.array_equal(run.arr("h", 1, "out"), run.arr("h", 1, "ref"))
    log = read_log(str(tmp_path))
    assert sum(1 for name, f in log if name == "ncclReduce") == 6       # the failed call is logged, and nothing else went wrong
    assert not [e for e in log if e[0].startswith("ERROR")]


def visible_devices(hk):
    """hipGetDeviceCount of the HIP runtime the library already loaded.  (Not torch: importing torch here would map torch's own HIP runtime
    and librccl into the test process, and the library's later dlopen("librccl.so.1") would pick that one up.)"""
    hk._lib.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line.split()[-1]}, key=lambda p: "/torch/" in p)
    assert paths, "the library maps no HIP runtime"
    n = ctypes.c_int(0)
    assert ctypes.CDLL(paths[0]).hipGetDeviceCount(ctypes.byref(n)) == 0
    return n.value


@pytest.mark.gpu
def test_i_local_comm_over_two_devices(hk, double_dir, tmp_path):
    """hk_comm_create over two contexts of one process (the Julia shim's layout): GroupStart, one ncclReduce per device, GroupEnd"""
    n = visible_devices(hk)
    if n < 2:
        pytest.skip("hk_comm_create needs two devices (one context per device); this box has %d" % n)
    scen = [{"name": "i", "root": 0, "samples": 8}]
    run = Run(str(tmp_path), 2, run_workers(double_dir, str(tmp_path), 1, scen, local=True))
    run.check_reduced("i", root=0)
    log = read_log(str(tmp_path))
    groups = [(name, int(f["group"])) for name, f in log if name in ("ncclGroupStart", "ncclGroupEnd")]
    assert groups == [("ncclGroupStart", 1), ("ncclGroupEnd", 1)], groups
    assert [int(f["group"]) for name, f in log if name == "ncclReduce"] == [1, 1]

