"""STRIPE_SCHEDULE_EMU: the multi-rank launch schedules run on one rank.

split   run_pass's overlap branch (boundary rows on the comm stream beside the
        interior launch, joined by events), without the exchange
pipe    run_pipelined (core / rim / boundary rows on three streams)
split1  interior, then both boundary ranges, on one stream

Each value splits every step's rows into several launches, so the output must
still equal the golden path bit for bit.  The variable is read once per
process (schedule_emu() caches it), so every value runs in a fresh child.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 333 pixels: 999-byte RGB rows (a shortened last tile); 37 rows: more than
# 4 R for both filters (pipelined_ok) and no multiple of the 4-row step
W, H, ITERS = 333, 37, 3

CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["STRIPE_ROOT"])
import mpi_cuda_imagemanipulation_amd as m
C = m._C
W, H, ITERS = (int(v) for v in sys.argv[1:4])
for chain, cc in (("gaussian5", 3), ("sobel", 1)):
    info = C.plan_info(chain, cc)
    # what the emu branches ask of a chain: one iterable pass with 0 < 4 R < rows
    assert len(info["passes"]) == 1 and 0 < 4 * info["passes"][0]["R"] < H, info
    e = C.Engine(m.Pipeline(chain).config(W, H, cc, "device", device=0))
    e.load_synthetic(7)
    e.run(ITERS)
    got = e.store_packed()
    ref = m.utils.synthetic_image(7, W, H, cc)
    for _ in range(ITERS):
        ref = C.golden_apply(ref, chain, "reflect101", True)
    assert got.size == ref.size == W * H * cc, (chain, got.shape, ref.shape)
    bad = int((got.reshape(-1) != ref.reshape(-1)).sum())
    assert bad == 0, f"{chain}: {bad} bytes differ from the golden path"
    del e
print("emu ok", os.environ["STRIPE_SCHEDULE_EMU"])
'''


@pytest.mark.parametrize("emu", ["split", "pipe", "split1"])
def test_schedule_emu_matches_golden(tmp_path, emu):
    script = tmp_path / "emu_child.py"
    script.write_text(CHILD)
    env = dict(os.environ, STRIPE_ROOT=ROOT, STRIPE_SCHEDULE_EMU=emu)
    r = subprocess.run([sys.executable, str(script), str(W), str(H), str(ITERS)], env=env, capture_output=True,
                       text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert f"emu ok {emu}" in r.stdout
