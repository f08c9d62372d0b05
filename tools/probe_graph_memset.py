"""Does a memset node of a captured graph still write its value when the graph is replayed after other work on the device?

Part 1 needs nothing of this library: a graph that holds ONE ``hipMemsetAsync(buf, value, n)`` (through ctypes on the HIP runtime) is
replayed after the buffer was poisoned in different ways, and the bytes it leaves are counted.  Part 2 captures ``sx_deconv_quantify`` (a
memset and one kernel) as tests/test_quantify_gpu.py does and replays it in that test's order, in that order with one more small
launch in front of each replay, and without the eager ``sx_deconv_quantify`` between the replays.  Prints one line per scenario; nothing is asserted.
    python tools/probe_graph_memset.py [--out profiles/graph_memset_probe.txt]"""
from __future__ import annotations

import argparse
import ctypes
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import _native, stain_basis  # noqa: E402
from tools.bench_masked import real_batch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "graph_memset_probe.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    loaded = [line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line]      # (the runtime torch loaded, not a second copy)
    hip = ctypes.CDLL(loaded[0] if loaded else "libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    lines = [f"device {torch.cuda.get_device_name(dev)}, torch {torch.__version__}, HIP {torch.version.hip}", ""]

    def say(text: str) -> None:
        print(text)
        lines.append(text)

    def capture(body):
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            body(_native.stream_ptr(dev))
        return graph

    # ---- part 1: a graph of one memset node ----
    say("part 1: a captured graph of ONE hipMemsetAsync(buf, value, 4096); wrong bytes inside the range after each replay")
    nbytes = 4096
    other = torch.zeros(1024, device=dev)
    host = torch.full((nbytes,), 0xA5, dtype=torch.uint8).pin_memory()

    def by_kernel(buf):
        buf.fill_(0xA5)

    def by_memset(buf):
        assert hip.hipMemsetAsync(buf.data_ptr(), 0xA5, nbytes, _native.stream_ptr(dev)) == 0

    def by_copy(buf):
        buf.copy_(host, non_blocking=True)

    def kernel_elsewhere(buf):
        other.add_(1.0)

    for value in (0, 3):
        for name, poison in (("nothing between the replays", None), ("buffer poisoned by a kernel (fill_)", by_kernel), ("buffer poisoned by an eager hipMemsetAsync", by_memset),
                             ("buffer poisoned by a copy from pinned host memory", by_copy), ("a kernel on another tensor", kernel_elsewhere)):
            buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
            graph = capture(lambda s, buf=buf, value=value: hip.hipMemsetAsync(buf.data_ptr(), value, nbytes, s))
            wrong = []
            for _ in range(4):
                if poison is not None:
                    poison(buf)
                graph.replay()
                torch.cuda.synchronize()
                wrong.append(int((buf != value).sum()))      # (the check itself launches kernels: "nothing" means nothing BEFORE the first count)
            say(f"  value {value}, {name:52s} wrong bytes per replay {wrong}")
    buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    graph = capture(lambda s: hip.hipMemsetAsync(buf.data_ptr(), 0, nbytes, s))
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize()
    say(f"  value 0, four replays back to back, counted once at the end      wrong bytes {int((buf != 0).sum())}")

    # ---- part 2: sx_deconv_quantify captured, as tests/test_quantify_gpu.py::test_a_captured_call_reads_new_pixels_at_replay ----
    say("")
    say("part 2: sx_deconv_quantify (a memset and one kernel) captured; is the (2, 772) output of each replay the eager call's?")
    lib = _native.require()
    f32 = _native.DTYPE_CODES[torch.float32]
    tiles = real_batch(4, 256, torch.float32)[:, :, :160, :112].contiguous().to(dev)
    first, second = tiles[:2].contiguous(), tiles[2:].contiguous()
    basis = stain_basis("hed").to(dev)

    def quantify(x, out, stream):
        assert lib.sx_deconv_quantify(x.data_ptr(), f32, 2, 160, 112, basis.data_ptr(), 1, 5, 64, 1, out.data_ptr(), 0, stream) == 0

    def eager(x):
        out = torch.empty((2, 772), dtype=torch.int64, device=dev)
        quantify(x, out, _native.stream_ptr(dev))
        return out

    want = {"first": eager(first), "second": eager(second)}
    torch.cuda.synchronize()

    def small_launch():
        other.add_(1.0)

    # (the test's order: replay, synchronise, an eager sx_deconv_quantify of the replayed tiles with torch.cat and torch.equal, x.copy_(), replay)
    for name, before_replay in (("the test's order: eager quantify + cat + equal, x.copy_(), replay", None),
                                ("the test's order with ONE small launch (add_ on another tensor) in front of each replay", small_launch),
                                ("no eager quantify: equal against rows computed beforehand, x.copy_(), replay", "skip"),
                                ("the test's order with a fresh torch.zeros(8).add_(1) in front of each replay", lambda: torch.zeros(8, device=dev).add_(1)),
                                ("the test's order, and the differing words COUNTED after each replay ((out != rows).sum())", "count")):
        x = first.clone()
        out = torch.empty((2, 772), dtype=torch.int64, device=dev)
        out.view(torch.uint8).fill_(0xA5)
        graph = capture(lambda s, x=x, out=out: quantify(x, out, s))
        wrong = []
        for which in ("first", "second", "first", "second"):
            x.copy_(first if which == "first" else second)
            if callable(before_replay):
                before_replay()
            graph.replay()
            torch.cuda.synchronize(dev)
            rows = want[which] if before_replay == "skip" else torch.cat([t.reshape(2, -1) for t in (eager(first if which == "first" else second),)], dim=1)
            wrong.append(bool(torch.equal(out, rows)))      # (nothing else is launched: the test's order is kept)
            if before_replay == "count":
                wrong[-1] = int((out != rows).sum()) == 0
        say(f"  {name:92s} replay equals the eager rows {wrong}")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
