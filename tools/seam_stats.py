"""The seam between two frames in a kernel trace (the kernel_trace_tail.csv of tools/gpu_trace.sh): per kernel of the stretch from the
end-of-frame prediction's resolve to the next frame's first tracking launch, the median over the steady-state frames of its summed
duration and launch count per frame.  tools/frame_timeline.py --list shows one such frame in order.
usage: seam_stats.py <csv>"""
import csv, statistics, sys

SEAM = ["splat_resolve_kernel", "fill_ratio_kernel", "fill_in_kernel", "prep_fused_kernel", "rgbd_pyrdown_kernel"]
AFTER = ["frame_maps_kernel", "so3_prealign_kernel"]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    so3 = [i for i, r in enumerate(rows) if "so3_prealign" in r["name"]]
    per = {n: [] for n in SEAM + AFTER}
    cnt = {n: [] for n in SEAM + AFTER}
    period = []
    for a, b in zip(so3[3:-1], so3[4:]):
        fr = rows[a:b]
        period.append(int(rows[b]["start_ns"]) - int(rows[a]["start_ns"]))
        for n in per:
            xs = [int(r["end_ns"]) - int(r["start_ns"]) for r in fr if n in r["name"]]
            per[n].append(sum(xs)); cnt[n].append(len(xs))
    print(f"frames {len(period)}: period median {statistics.median(period) / 1e3:.1f} us")
    total = 0.0
    for n in SEAM + AFTER:
        m = statistics.median(per[n]) / 1e3
        print(f"  {n:24s} {m:7.1f} us per frame (median of sums), {int(statistics.median(cnt[n]))} launches")
        if n in SEAM:
            total += m
    print(f"  the first {len(SEAM)} rows, total {total:.1f} us")


if __name__ == "__main__":
    main()
