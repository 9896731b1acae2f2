"""Calls havoc_mi355x_sao_apply 10 times at 1080p 8-bit CTB 64 and at 2160p 10-bit CTB 64 / 16, for
rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r06/sao_apply_prof.py  (from the repository root;
sao_apply_kernel_times.txt holds the result)."""
import sys, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import sao_apply_tools as A
from turingcodec_amd.havoc import Havoc
hv = Havoc(stream="new")
torch = hv.torch
for (W, H, bd, log2) in ((1920, 1080, 8, 6), (3840, 2160, 10, 6), (3840, 2160, 10, 4)):
    cx, cy = -(-W >> log2), -(-H >> log2)
    rng = np.random.default_rng(W + log2)
    dec = A.random_decisions(rng, cx * cy, bd, dense=True)
    dt = np.uint8 if bd == 8 else np.uint16
    ry = hv.up(rng.integers(0, 1 << bd, W * H).astype(dt))
    rc = hv.up(rng.integers(0, 1 << bd, W * H // 2).astype(dt))
    with torch.cuda.stream(hv.tstream):
        oy, oc = torch.zeros_like(ry), torch.zeros_like(rc)
        d = torch.from_numpy(dec.view(np.uint8).reshape(-1).copy()).to(hv.device)
        blk = torch.full(((H + 7) // 8 * ((W + 7) // 8),), 60, dtype=torch.int8, device=hv.device)
    nc = W * H // 4
    for _ in range(10):
        hv.sao_apply_d(bd, 3, W, H, log2, ry, 0, rc, 0, nc, W, W // 2, oy, 0, oc, 0, nc, W, W // 2, d, None, blk, (W + 7) // 8)
    hv.sync()
    print("ok", W, H, bd, 1 << log2)
