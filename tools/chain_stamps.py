"""Phase stamps of the prior (0-7) and the stage (8-15) of the two-pass Macenko transform on config 2, rotating over two
batches as bench.py does: per phase (stamp k -> k + 1) the median and the slowest tile, in us.  Needs the diagnostic build
(STAINX_DIAG=1, or STAINX_HIP_LIB naming one).    python tools/chain_stamps.py [calls]"""
import sys, torch
sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from stainx_amd import synth
from stainx_amd.backends.torch_hip_backend import MacenkoHIP

dev = torch.device("cuda:0")
be = MacenkoHIP(dev)
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
xs = [synth.as_dtype(synth.he_batch(64, 512, 512, seed0=1000 + 64 * b), torch.float32).to(dev) for b in range(2)]
he, mc = be.compute_reference_stain_matrix(synth.reference_tile(512, 512).to(dev))
for i in range(10):
    be.transform(xs[i & 1], he, mc)
deltas = []
for i in range(calls):
    be.transform(xs[i & 1], he, mc)
    torch.cuda.synchronize()
    p = be.tile_params(64)
    s = p["stamps_us"].double()
    deltas.append(torch.cat([s[:, 1:8] - s[:, 0:7], s[:, 9:16] - s[:, 8:15]], 1))
    n_cand, fell = p["n_candidates"], p["fell_back"]
d = torch.stack(deltas)                      # calls x tiles x 14
med = d.median(0).values                     # per tile, over the calls
names = [f"{k}->{k + 1}" for k in range(7)] + [f"{k}->{k + 1}" for k in range(8, 15)]
print("phase      median  slowest-tile   (us; per tile the median over %d calls)" % calls)
for k, nm in enumerate(names):
    print(f"{nm:8s} {med[:, k].median().item():8.2f} {med[:, k].max().item():8.2f}")
print(f"prior 0->7 {med[:, :7].sum(1).median().item():.2f} / {med[:, :7].sum(1).max().item():.2f}   stage 8->15 {med[:, 7:].sum(1).median().item():.2f} / {med[:, 7:].sum(1).max().item():.2f}")
print("candidates per slot: mean", [round(float(v), 1) for v in n_cand.double().mean(0)], "sum", [int(v) for v in n_cand.sum(0)], " tiles with a slow slot:", int((fell & 15 != 0).sum()))
