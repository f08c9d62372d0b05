"""One Macenko.transform of 64 x 3 x 512 x 512 float32 (the headline's shape, two rotating batches), device time per call, on
  * the headline's tiles (u8 / 255: every tile coded -- 4-byte code records between pass A and the estimate stage), and
  * the same tiles after a sub-LSB perturbation (ordinary floats: the prior finds every tile not coded, pass A attempts no lookup).
The loaded library is STAINX_HIP_LIB's, or the tree's; to compare two builds run it once per library in ONE session, alternating:
    STAINX_HIP_LIB=/path/to/parent/libstainx_hip.so python tools/ab_code_records.py [calls]
    python tools/ab_code_records.py [calls]
Prints one line per batch kind: median and minimum over the calls, and the number of tiles with a slow slot in the last call."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stainx_amd import _native, synth
from stainx_amd.backends.torch_hip_backend import MacenkoHIP

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
dev = torch.device("cuda", 0)
sm = torch.tensor(synth.HE_REF, dtype=torch.float32)
tmc = torch.tensor([1.9705, 1.0308], dtype=torch.float32)


def time_it(be, batches):
    for i in range(30):
        be.transform(batches[i % 2], sm, tmc)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for i in range(calls):
        ev[i][0].record()
        be.transform(batches[i % 2], sm, tmc)
        ev[i][1].record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    p = be.tile_params(batches[0].shape[0])
    return t[len(t) // 2] * 1e3, t[0] * 1e3, int(((p["fell_back"] & 15) != 0).sum()), int(p["n_candidates"].sum())


levels = [synth.as_dtype(synth.he_batch(64, 512, 512, seed0=1000 + 64 * b), torch.float32) for b in range(2)]
g = torch.Generator().manual_seed(11)
floats = [(x + (torch.rand(x.shape, generator=g) - 0.5) * 1e-3).clamp_(0.0, 1.0) for x in levels]      # +-5e-4: an eighth of a grey level's spacing
lib = os.environ.get("STAINX_HIP_LIB", "the tree's library")
for name, batches in (("8-bit levels", levels), ("ordinary floats", floats)):
    be = MacenkoHIP(dev)      # (a backend of its own: the router's feedback of one kind says nothing about the other)
    med, best, slow, cand = time_it(be, [x.to(dev) for x in batches])
    print(f"{lib}: 64x3x512x512 f32 {name:16s} median {med:7.1f} us   min {best:7.1f} us   tiles with a slow slot {slow}   candidates {cand}   two-pass {int(cand > 0 and be._classic_left == 0)}", flush=True)
