"""The surfel passes that extent culling touches, in a kernel trace (the kernel_trace_tail.csv of tools/gpu_trace.sh): per kernel the median
over the steady-state frames of its summed duration and launch count per frame, in the manner of tools/seam_stats.py.  The two
index_resolve_kernel launches of a frame are listed apart (the second one also packs the clean stage's records).  Every other kernel name
of the frame is listed with its launch count, so that a launch the change added (a fill, say) shows.
usage: extent_stats.py <csv>"""
import collections, csv, statistics, sys

NAMES = ["index_splat_kernel", "indexsplat_scatter_kernel", "index_resolve_kernel", "splat_raster_kernel", "splat_resolve_kernel", "prep_fused_kernel",
         "clean_kernel", "associate_kernel"]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    so3 = [i for i, r in enumerate(rows) if "so3_prealign" in r["name"]]
    per = collections.defaultdict(list)
    cnt = collections.defaultdict(list)
    period, launches = [], []
    for a, b in zip(so3[3:-1], so3[4:]):
        fr = rows[a:b]
        period.append(int(rows[b]["start_ns"]) - int(rows[a]["start_ns"]))
        launches.append(len(fr))
        seen = collections.Counter()
        tot = collections.Counter()
        for r in fr:
            n = next((k for k in NAMES if k in r["name"]), r["name"].split("(")[0][:40])
            d = int(r["end_ns"]) - int(r["start_ns"])
            if n == "index_resolve_kernel":
                seen[n] += 1
                n = f"index_resolve_kernel #{seen[n]}"
            tot[n] += d
            seen[n] += 1
        for n in tot:
            per[n].append(tot[n]); cnt[n].append(seen[n])
    nf = len(period)
    print(f"frames {nf}: period median {statistics.median(period) / 1e3:.1f} us, {int(statistics.median(launches))} launches per frame")
    listed = [n for n in sorted(per) if any(k in n for k in NAMES)]
    for n in listed:
        print(f"  {n:30s} {statistics.median(per[n]) / 1e3:7.1f} us per frame (median of sums), {int(statistics.median(cnt[n]))} launches, in {len(per[n])} frames")
    print("  every other kernel: " + ", ".join(f"{n} x{int(statistics.median(cnt[n]))}" for n in sorted(per) if n not in listed and len(per[n]) * 2 > nf))


if __name__ == "__main__":
    main()
