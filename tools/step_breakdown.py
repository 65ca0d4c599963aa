"""Per-launch / per-stage breakdown of the last default-path vocoder step from a rocprofv3
kernel trace (bench.py --no-full --no-streaming ...; tools/prof_fused.sh).

usage: python tools/step_breakdown.py <trace dir>/run_kernel_trace.csv [B T] [--separate-up]
(--separate-up: the trace of a run with TTS_UP_FUSE=0, or of a library from before the stage 2-3
upsamplers moved into the preceding pair launches: "s2.up" / "s3.up" are launches of their own)
Labels come from tools/pmc_traffic.fused_step_layers (pre, ups, stage-0 convs, ResBlock
pairs, post); FLOPs are algorithmic (2*M*Cin*k per produced row; a pair counts both convs).
"""
import csv
import os
import sys
from collections import OrderedDict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.pmc_traffic import family, step_launches  # noqa: E402


def main():
    argv = [a for a in sys.argv if a != "--separate-up"]
    path = argv[1]
    B = int(argv[2]) if len(argv) > 2 else 32
    T = int(argv[3]) if len(argv) > 3 else 862
    rows = [r for r in csv.DictReader(open(path)) if family(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    step = step_launches(B, T, up_fused=()) if "--separate-up" in sys.argv else step_launches(B, T)
    rows = rows[-len(step):]
    stage = OrderedDict()
    total = 0.0
    print(f"{'launch':12s} {'kernel':10s} {'us':>9s} {'TF/s':>8s}")
    for (lab, _, f), r in zip(step, rows):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        total += us
        s = stage.setdefault(lab.split(".")[0], [0.0, 0.0])
        s[0] += us
        s[1] += f
        print(f"{lab:12s} {family(r['Kernel_Name']):10s} {us:9.1f} {f / (us * 1e-6) / 1e12:8.1f}")
    print()
    for st, (us, f) in stage.items():
        print(f"stage {st:5s} {us:9.1f} us  {f / (us * 1e-6) / 1e12:7.1f} TF/s  {100 * us / total:5.1f} %")
    print(f"step total {total:.1f} us")


if __name__ == "__main__":
    main()
