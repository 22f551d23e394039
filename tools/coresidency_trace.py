#!/usr/bin/env python
"""Developer tool: where the scale factors' background kernel runs relative to the two big kernels of the step, from a rocprofv3
kernel trace of bench.py (--kernel-trace --output-format csv).   python tools/coresidency_trace.py kernel_trace.csv [STEPS]

Over the last STEPS steps (default 1000: the timed loop): the durations of acc_dot_ctx_kernel, element_stats_stream_fused_kernel and
suffstats_chunk_stage1; the dot kernel's duration split by whether a stage-1 launch overlapped it; which kernel of the main stream
runs when a stage-1 launch begins and ends, and how much of the stage-1 interval lies inside the dot kernel's."""
import csv
import sys


def med(x):
    x = sorted(x)
    return x[len(x) // 2] if x else float("nan")


def st(x):
    x = sorted(x)
    return "n=%d median %.1f min %.1f p10 %.1f p90 %.1f max %.1f" % (len(x), med(x), x[0], x[len(x) // 10], x[len(x) * 9 // 10], x[-1]) if x else "n=0"


def main(path, steps):
    rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(path))]
    pick = lambda key: sorted([(a, b) for k, a, b in rows if key in k])[-steps:]
    # the DOT stage's kernel: element_p_stream_kernel where the plans stream a planned P (DIG_PIPE_ELEMENT_P; acc_dot_ctx_kernel then
    # runs once per plan, outside the timed loop), else acc_dot_ctx_kernel
    dot_name = "element_p_stream_kernel" if len(pick("element_p_stream_kernel")) >= steps else "acc_dot_ctx_kernel"
    dot, stat, bg = pick(dot_name), pick("element_stats_stream_fused"), pick("suffstats_chunk_stage1")
    t0 = dot[0][0]
    bg = [x for x in bg if x[1] > t0]
    us = lambda iv: [(b - a) / 1e3 for a, b in iv]
    print("last %d steps" % steps)
    print("%-29s us:" % dot_name, st(us(dot)))
    print("element_stats_stream_fused    us:", st(us(stat)))
    print("suffstats_chunk_stage1        us:", st(us(bg)))
    print("step period (dot start to dot start) us:", st([(b[0] - a[0]) / 1e3 for a, b in zip(dot, dot[1:])]))
    ov = lambda x, y: max(0, min(x[1], y[1]) - max(x[0], y[0]))
    met, alone, share = [], [], []
    j = 0
    for d in dot:
        while j < len(bg) and bg[j][1] <= d[0]:
            j += 1
        o = sum(ov(d, b) for b in bg[j:j + 3])
        (met if o > 0 else alone).append((d[1] - d[0]) / 1e3)
        share.append(o / float(d[1] - d[0]))
    print("dot kernel overlapped by stage 1  us:", st(met))
    print("dot kernel not overlapped         us:", st(alone))
    print("share of the dot kernel's interval covered by stage 1: median %.2f" % med(share))
    main_iv = sorted([(a, b, "dot") for a, b in dot] + [(a, b, "stat") for a, b in stat])

    def where(t):
        for a, b, name in main_iv:
            if a <= t < b:
                return name, (t - a) / float(b - a)
        return "gap", 0.0
    for label, pos in (("begins", 0), ("ends", 1)):
        c = {"dot": [], "stat": [], "gap": []}
        for b in bg:
            name, frac = where(b[pos])
            c[name].append(frac)
        print("stage 1 %s inside: dot %d (median phase %.2f)  statistics %d (median phase %.2f)  between kernels %d" %
              (label, len(c["dot"]), med(c["dot"]), len(c["stat"]), med(c["stat"]), len(c["gap"])))
    spans = sum(1 for b in bg if any(b[0] <= d[0] and b[1] >= d[1] for d in dot))
    print("stage-1 launches that span a whole dot kernel: %d of %d" % (spans, len(bg)))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1000)
