"""The multi-process DEVICE path on a one-GPU box (gloo-gpu backend).

The driver's scaling runs use one process per GPU over RCCL; a one-GPU box
cannot host that (RCCL refuses two ranks on one device), so the same
per-process device flow -- DistributedPipeline, scatter / halo exchange /
gather, the pipelined and weighted dist steps, the reference window into a
shared-memory frame, the cache-cold scope, bench.py's verification -- runs here
with N processes sharing GPU 0 and gloo moving the bytes through pinned host
memory (StagedComm).  This is also the reference's own deployment: every MPI
rank on GPU 0 (kernel.cu:147).
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _torchrun(n, args, tmp_path, timeout=300):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), *args]
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("n", [2, 4])
def test_bench_gloo_gpu_processes(tmp_path, n):
    recs = _torchrun(n, [os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--backend", "gloo-gpu",
                         "--width", "2048", "--height", "1536", "--steps", "6", "--warmup", "2",
                         "--full", "--dist-steps", "2", "--ref-steps", "2", "--e2e-steps", "2"], tmp_path)
    assert len(recs) == 1
    rec = recs[0]
    assert rec["n_gpus"] == n and rec["value"] > 0 and rec["verified_vs_golden"] is True
    assert sum(rec["stripe_rows"]) == 1536
    # the four halo schedules differ on device engines: each was timed on the
    # real transport and the verified headline ran the fastest
    # (frames rotate here, so one stream and two alternating ones are both
    # tried; processes sharing one GPU take plain streams only --
    # dedicated hardware queues in every process oversubscribe the GPU's queue
    # slots, profiles/r5/shared/ -- otherwise both stream sets are tried)
    import torch

    hs = rec["halo_schedule"]
    # (768- / 384-row stripes: an auto halo depth of 4 / 2, so the deep
    # schedules are candidates too)
    scheds = ("serial", "overlap", "pipeline", "batched", "ahead", "serial+deep", "batched+deep", "ahead+deep")
    if n > torch.cuda.device_count():
        assert hs["queues"] == "plain"
        assert set(hs["ms"]) == {f"{s}@{k}" for s in scheds for k in (1, 2)}
    else:
        assert set(hs["ms"]) == ({f"{s}@1" for s in scheds} |
                                 {f"{s}@2/{q}" for s in scheds for q in ("dedicated", "plain")})
    multi = any("/" in k for k in hs["ms"])
    key = f"{hs['chosen']}@{hs['streams']}" + (f"/{hs['queues']}" if hs["streams"] > 1 and multi else "")
    assert key == min(hs["ms"], key=hs["ms"].get) and rec["streams"] == hs["streams"]
    assert (rec["halo_depth"] > 1) == ("+deep" in hs["chosen"])  # the record names the depth the steps ran
    for name, sc in rec["scopes"].items():
        assert "error" not in sc, (name, sc)
        if "verified" in sc:
            assert sc["verified"] is True, (name, sc)


@pytest.mark.parametrize("extra", [["--dist-chunks", "4"], ["--preset", "ref-gpu"],
                                   ["--dist-chunks", "2", "--row-weights", "0.5,0.2,0.2,0.1"]])
def test_cli_gloo_gpu_4_processes(tmp_path, C, extra):
    import mpi_cuda_imagemanipulation_amd as m

    img = m.utils.synthetic_image(11, 301, 203, 3)
    src, out = tmp_path / "in.ppm", tmp_path / "out.ppm"
    m.utils.write_image(str(src), img)
    args = ["-m", "mpi_cuda_imagemanipulation_amd", "run", "--input", str(src), "--output", str(out),
            "--backend", "gloo-gpu", *extra]
    if "--preset" not in extra:
        args += ["--chain", "gaussian5"]
    recs = _torchrun(4, args, tmp_path)
    assert len(recs) == 1 and recs[0]["ranks"] == 4
    got = m.utils.read_image(str(out))
    if "--preset" in extra:
        import np_ref

        rows = 203 // 4
        for r in range(4):
            s = img[r * rows:(r + 1) * rows]
            e = np_ref.stencil(np_ref.contrast_ref(np_ref.gray_ref(s), 3.5), "emboss3", "skip")
            assert (got[r * rows:(r + 1) * rows] == np_ref.expand(e)).all(), r
    else:
        assert (got == C.golden_apply(img, "gaussian5", "reflect101", True)).all()


SCHED_WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["STRIPE_ROOT"])
from mpi_cuda_imagemanipulation_amd import parallel, models
from mpi_cuda_imagemanipulation_amd._native import C
ctx = parallel.init("gloo-gpu")
W, H, Cc, chain = 700, 256, 3, "gaussian5"
fs = parallel.FrameStream(ctx, models.Pipeline(chain, halo_depth=1), W, H, Cc, frames=2, streams=2)
row0, rows = fs.head.stripe
fs.tune()
refs = []
for f in range(2):
    ref = C.synth_image(5 + f, W, H, Cc)
    for _ in range(3):
        ref = C.golden_apply(ref, chain, "reflect101", True)
    refs.append(ref[row0:row0 + rows])
bad = []
for sched in ("serial", "overlap", "pipeline"):
    for ns in (1, 2):
        fs.set_schedule(sched)
        fs.set_streams(ns)
        fs.load_synthetic(5)
        for _ in range(6):
            fs.step()
        fs.synchronize()
        for f in range(2):
            if not (fs.frames[f].result_stripe() == refs[f]).all():
                bad.append([sched, ns, f])
# one file per rank: the ranks share torchrun's stdout, where their writes can
# interleave character by character
with open(f"result_{ctx.rank}.json", "w") as fh:
    json.dump(bad, fh)
# explicit teardown: engines (and their communicator) before the process
# group, every rank together, so no gloo work or thread outlives it at exit
import gc, torch, torch.distributed as dist
del fs
gc.collect()
torch.cuda.synchronize()
dist.barrier()
dist.destroy_process_group()
'''


def test_frame_stream_every_schedule_exact_gloo_gpu(tmp_path):
    # pick_schedule may choose any schedule x stream count on the real
    # transport, so every combination must be exact across ranks: 2 processes,
    # 2 frames, 3 iterated steps each, vs the golden path
    script = tmp_path / "w.py"
    script.write_text(SCHED_WORKER)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), str(script)]
    env = dict(os.environ, STRIPE_ROOT=ROOT, OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    for rank in (0, 1):
        f = tmp_path / f"result_{rank}.json"
        assert f.exists(), (rank, r.stdout[-2000:])
        assert json.loads(f.read_text()) == [], rank
