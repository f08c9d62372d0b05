"""Kernel-trace target for comparing the launches of two builds: every Reinhard / histogram-matching / tissue-mask / luminosity-apply
entry point once (the calls of host_layer_fingerprint.py's siblings(), explicit masks only), float32, at 2 x 3 x 48 x 48 and 16 x 3 x 512 x 512.
    STAINX_HIP_LIB=/path/to/libstainx_hip.so rocprofv3 --kernel-trace --output-format csv -d out -o kt -- python tools/sibling_launches.py
    python tools/sibling_launches.py --table out/.../kt_kernel_trace.csv > launches.txt      # kernel, grid, workgroup: one line per launch, in order
Two builds that launch the same kernels in the same order on the same grids give identical tables (names without template arguments
that only one build has are a difference: the table shows it)."""
import csv, os, re, sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def table(path):
    rows = list(csv.DictReader(open(path)))
    cols = list(rows[0])
    start = next(c for c in cols if c.lower().startswith("start"))
    grid, group = sorted(c for c in cols if c.lower().startswith("grid_size")), sorted(c for c in cols if c.lower().startswith("workgroup_size"))
    rows.sort(key=lambda r: int(r[start]))
    for r in rows:
        if "sx::" in r["Kernel_Name"]:      # (the library's own launches: torch's fills and copies of the driver are not the subject)
            print(re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void sx::", ""), "grid", *[r[c] for c in grid], "workgroup", *[r[c] for c in group])


def main():
    if sys.argv[1:2] == ["--table"]:
        return table(sys.argv[2])
    import torch
    import host_layer_fingerprint as fp
    from stainx_amd import _native

    lib = _native._open(Path(os.environ.get("STAINX_HIP_LIB", _native.LIB_PATH)).resolve())
    g = fp.Gpu(lib)
    for n, h, w in ((2, 48, 48), (16, 512, 512)):
        fp.siblings(g, f"float32 {n}x{h}x{w}", torch.float32, n, h, w, masks=("half",))
    failed = sorted(k for k, v in g.out.items() if v["rc"] != 0)
    print(f"{len(g.out)} calls, {len(failed)} failed", *failed, sep="\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
