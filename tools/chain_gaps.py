"""Per-kernel mean and the gaps between the four launches of a two-pass Macenko call, from a rocprofv3 kernel trace
(`*_kernel_trace.csv` under the given directory: tools/prof_headline.sh leaves one).

    python tools/chain_gaps.py <trace_dir> [calls_to_skip]

A call is prior -> pass A -> stage -> reconstruct on one stream; gaps are next start - previous end.  "chain" is what a call
spends with most of the chip idle: prior + stage + the three gaps inside the call."""
import csv
import glob
import statistics as st
import sys

ORDER = ("prior_kernel", "pass_a_kernel", "estimate_stage_kernel", "reconstruct_kernel")


def main():
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    rows = []
    for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = next((k for k in ORDER if k in r["Kernel_Name"]), None)
            if name and "float" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    calls, i = [], 0
    while i + 3 < len(rows):
        if tuple(r[2] for r in rows[i:i + 4]) == ORDER:
            calls.append(rows[i:i + 4])
            i += 4
        else:
            i += 1
    calls = calls[skip:]
    dur = {k: [] for k in ORDER}
    gaps = {"prior->A": [], "A->stage": [], "stage->recon": [], "call->call": []}
    chain, whole = [], []
    for n, c in enumerate(calls):
        for s, e, k in c:
            dur[k].append((e - s) / 1e3)
        g = [(c[k + 1][0] - c[k][1]) / 1e3 for k in range(3)]
        for key, v in zip(("prior->A", "A->stage", "stage->recon"), g):
            gaps[key].append(v)
        chain.append(dur["prior_kernel"][-1] + dur["estimate_stage_kernel"][-1] + sum(g))
        whole.append((c[3][1] - c[0][0]) / 1e3)
        if n + 1 < len(calls):
            nxt = (calls[n + 1][0][0] - c[3][1]) / 1e3
            if nxt < 100.0:      # (the loops of a run are apart by more)
                gaps["call->call"].append(nxt)
    print(f"{len(calls)} calls")
    for k in ORDER:
        print(f"{k:24s} mean {st.mean(dur[k]):6.2f} us  median {st.median(dur[k]):6.2f}  sd {st.pstdev(dur[k]):5.2f}")
    for k, v in gaps.items():
        print(f"gap {k:20s} mean {st.mean(v):6.2f} us  median {st.median(v):6.2f}")
    a_r = [a + r for a, r in zip(dur["pass_a_kernel"], dur["reconstruct_kernel"])]
    print(f"pass A + reconstruct     mean {st.mean(a_r):6.2f} us  sd {st.pstdev(a_r):5.2f}")
    print(f"chain (prior + stage + three gaps) mean {st.mean(chain):6.2f} us  median {st.median(chain):6.2f}")
    print(f"first start -> last end  mean {st.mean(whole):6.2f} us  median {st.median(whole):6.2f}")


if __name__ == "__main__":
    main()
