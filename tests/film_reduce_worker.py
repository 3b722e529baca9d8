"""One rank of tests/test_film_reduce_ranks.py, run as a script: python film_reduce_worker.py SPEC.json RANK.

It loads librccl.so.1 from the test double's directory (LD_LIBRARY_PATH, set by the parent) and never imports torch (torch would map
the real librccl).  Rank 0 writes the communicator's unique id to a file in the spec's directory; every rank then creates its rank of
the communicator and runs the spec's scenarios in order.  Each scenario saves .npy arrays in the directory — the rank's reference film
(its share rendered and read back), the film after hk_film_reduce and, on the root, the whole frame rendered in one process — and the
parent compares them.  result_r<RANK>.json records, per scenario, how many ncclReduce calls this process made, and what the failure
scenarios returned."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402

import hikari_jl_amd as hk  # noqa: E402
from hikari_jl_amd import distributed as hd  # noqa: E402
from hikari_jl_amd import scenes  # noqa: E402

W, H = 67, 45   # ragged: neither is a multiple of the 8x8 path tile


def librccl_mappings():
    with open("/proc/self/maps") as f:
        return sorted({line.split()[-1] for line in f if "librccl" in line.split()[-1]})


def own_reduce_calls(log_path):
    """ncclReduce calls logged by this process (the double appends one line per call, synchronously, from the calling thread)"""
    if not os.path.exists(log_path):
        return []
    tag = "pid=%d " % os.getpid()
    with open(log_path) as f:
        return [line.split() for line in f if line.startswith("ncclReduce ") and tag in line]


def fields(tokens):
    return dict(t.split("=", 1) for t in tokens[1:] if "=" in t)


class Rank:
    def __init__(self, spec, rank):
        self.spec, self.rank, self.world = spec, rank, spec["world"]
        self.dir = spec["dir"]
        self.log = os.path.join(self.dir, "fake_rccl.log")
        self.ctx = hk.Context.get(0)
        self.result = {"rank": rank, "pid": os.getpid(), "scenarios": {}}

    def save(self, scenario, name, arr):
        np.save(os.path.join(self.dir, "%s_r%d_%s.npy" % (scenario, self.rank, name)), arr)

    def connect(self):
        uid_path = os.path.join(self.dir, "unique_id.bin")
        if self.rank == 0:
            uid = hk.Comm.unique_id()
            with open(uid_path + ".tmp", "wb") as f:
                f.write(uid)
            os.rename(uid_path + ".tmp", uid_path)
        else:
            end = time.monotonic() + 120
            while not os.path.exists(uid_path):
                assert time.monotonic() < end, "rank 0 never wrote the unique id"
                time.sleep(0.05)
            with open(uid_path, "rb") as f:
                uid = f.read()
        assert len(uid) == 128
        self.comm = hk.Comm.rank(self.ctx, uid, self.rank, self.world)
        # librccl was loaded by the calls above: from the double's directory and nowhere else
        maps = librccl_mappings()
        assert maps and all(os.path.dirname(p) == self.spec["double_dir"] for p in maps), maps
        self.result["librccl_maps"] = maps
        self.result["unique_id_magic"] = uid[:8].decode("latin-1")

    def connect_local(self):
        """hk_comm_create over cuda:0 and cuda:1 in this one process (world 2, ranks = devices)"""
        self.result["unique_id_magic"] = hk.Comm.unique_id()[:8].decode("latin-1")
        self.ctxs = [hk.Context.get(0), hk.Context.get(1)]
        self.comm = hk.Comm.local(self.ctxs)
        maps = librccl_mappings()
        assert maps and all(os.path.dirname(p) == self.spec["double_dir"] for p in maps), maps
        self.result["librccl_maps"] = maps

    def run_local(self, sc):
        name, root, n = sc["name"], sc["root"], sc["samples"]
        s, film, cam = self.scene("cornell")
        films = [hk.Film((W, H)) for _ in self.ctxs]
        vps = [hk.VolPath(max_depth=5, samples=n, device=r) for r in range(len(self.ctxs))]
        for r, vp in enumerate(vps):
            vp._ensure(films[r])
            vp.clear()
            first, count, stride = hd.shard_samples(n, r, len(vps))
            vp.render_samples(s, films[r], cam, count, stride=stride, first=first, readback=False)
            self.save_as(r, name, "ref", vp.read_accumulators(films[r]))
        for r, vp in enumerate(vps):
            vp.clear()
            first, count, stride = hd.shard_samples(n, r, len(vps))
            vp.render_samples(s, films[r], cam, count, stride=stride, first=first, readback=False)
        self.comm.reduce_films(vps, root=root)
        for r, vp in enumerate(vps):
            self.save_as(r, name, "out", vp.read_accumulators(films[r]))
            vp.close()
        whole = hk.VolPath(max_depth=5, samples=n, device=root)
        whole(s, film, cam)
        self.save_as(root, name, "whole", whole.read_accumulators(film))
        whole.close()
        self.result["scenarios"][name] = {}

    def save_as(self, rank, scenario, name, arr):
        np.save(os.path.join(self.dir, "%s_r%d_%s.npy" % (scenario, rank, name)), arr)

    # -- scenarios ---------------------------------------------------------------------------------------------------------------
    def scene(self, which):
        if which == "cornell":
            s, film, cam = scenes.cornell_box(W, H, light="area")
        else:   # a fog-filled glass sphere: ticketed medium segments
            s, _, _ = scenes.integration_test_scene(W, H)
            film = hk.Film((W, H))
            cam = hk.PerspectiveCamera((0, 1, -3.5), (0, 1, 0), film, fov=40.0)
        return s, film, cam

    def integrator(self, sc, samples):
        filt = hk.BoxFilter() if sc.get("filter") == "box" else None
        return hk.VolPath(max_depth=5, samples=samples, filter=filt, accumulation_eltype="Float64" if sc.get("f64") else "Float32")

    def render_share(self, sc, vp, s, film, cam):
        """this rank's share of the frame, enqueued without any read-back or sync"""
        n = sc["samples"]
        if sc.get("tiles"):
            vp.render_samples(s, film, cam, n, first=1, tile=hd.shard_tiles(W, H, self.rank, self.world), readback=False)
            return
        first, count, stride = hd.shard_samples(n, self.rank, self.world)
        if sc.get("one_sample_calls"):
            for i in range(count):
                vp.render_samples(s, film, cam, 1, stride=stride, first=first + i * stride, readback=False)
        elif count:
            vp.render_samples(s, film, cam, count, stride=stride, first=first, readback=False)

    def run(self, sc):
        name, root = sc["name"], sc["root"]
        before = len(own_reduce_calls(self.log))
        s, film, cam = self.scene(sc.get("scene", "cornell"))
        vp = self.integrator(sc, sc["samples"])
        vp._ensure(film)
        with self.ctx.options(**sc.get("knobs", {})):
            vp.clear()
            self.render_share(sc, vp, s, film, cam)
            self.save(name, "ref", vp.read_accumulators(film))
            for _ in range(sc.get("frames", 1)):   # the bench loop: clear -> render -> reduce, no sync in between
                vp.clear()
                self.render_share(sc, vp, s, film, cam)
                self.comm.reduce_films([vp], root=root)
            extra = sc.get("extra_samples", 0) if self.rank == root else 0
            for i in range(extra):                 # work after the reduce, no sync: must be ordered behind its device copy
                vp.render_samples(s, film, cam, 1, first=sc["samples"] + 1 + i, readback=False)
            self.save(name, "out", vp.read_accumulators(film))
            if extra:
                vp.clear()
                for i in range(extra):
                    vp.render_samples(s, film, cam, 1, first=sc["samples"] + 1 + i, readback=False)
                self.save(name, "extra", vp.read_accumulators(film))
        vp.close()
        if self.rank == root:   # the whole frame, all samples in one process
            whole = self.integrator(sc, sc["samples"])
            film2 = hk.Film((W, H))
            whole(s, film2, cam)
            self.save(name, "whole", whole.read_accumulators(film2))
            whole.close()
        calls = own_reduce_calls(self.log)[before:]
        self.result["scenarios"][name] = {"reduces": [fields(c) for c in calls]}

    def run_injected_reduce_failure(self, sc):
        """FAKE_RCCL_FAIL=reduce:2 (set by the parent): the 2nd reduce of every rank fails, the 3rd on the same comm must be right"""
        name, root = sc["name"], sc["root"]
        s, film, cam = self.scene("cornell")
        vp = self.integrator(sc, sc["samples"])
        vp._ensure(film)
        vp.clear()
        self.render_share(sc, vp, s, film, cam)
        self.save(name, "ref", vp.read_accumulators(film))
        L = hk._lib.lib()
        films = (C.c_void_p * 1)(vp._film[0])
        codes, messages = [], []
        for _ in range(3):
            vp.clear()
            self.render_share(sc, vp, s, film, cam)
            codes.append(L.hk_film_reduce(self.comm.h, films, 1, root))
            messages.append(L.hk_last_error().decode() if codes[-1] else "")
            if codes[-1] == 0:
                out = vp.read_accumulators(film)
        self.save(name, "out", out)
        vp.close()
        self.result["scenarios"][name] = {"codes": codes, "messages": messages}

    def run_injected_initrank_failure(self):
        """FAKE_RCCL_FAIL=initrank: hk_comm_create_rank fails with HK_ERR_DEVICE and leaves the out pointer null"""
        os.environ["FAKE_RCCL_FAIL"] = "initrank"   # (the double reads it at every call)
        uid = (C.c_uint8 * 128).from_buffer_copy(hk.Comm.unique_id())
        L = hk._lib.lib()
        out = C.c_void_p()
        code = L.hk_comm_create_rank(self.ctx.h, uid, self.rank, self.world, C.byref(out))
        self.result["initrank"] = {"code": code, "message": L.hk_last_error().decode(), "out_is_null": out.value is None,
                                   "destroy_null": L.hk_comm_destroy(out)}
        del os.environ["FAKE_RCCL_FAIL"]


def main():
    with open(sys.argv[1]) as f:
        spec = json.load(f)
    rank = int(sys.argv[2])
    r = Rank(spec, rank)
    if spec.get("local"):
        r.connect_local()
    else:
        r.connect()
    for sc in spec["scenarios"]:
        if spec.get("local"):
            r.run_local(sc)
        elif sc.get("inject") == "reduce":
            r.run_injected_reduce_failure(sc)
        else:
            r.run(sc)
    r.comm.close()
    if spec.get("initrank_failure"):
        r.run_injected_initrank_failure()
    assert "torch" not in sys.modules, "the worker must not import torch (it maps the real librccl)"
    r.result["torch_imported"] = False
    with open(os.path.join(spec["dir"], "result_r%d.json" % rank), "w") as f:
        json.dump(r.result, f)
    print("rank %d ok" % rank)


if __name__ == "__main__":
    main()
