"""One steady-state null-space set-up launch by launch with the stream of every launch (development probe): kernel trace CSV of a
rocprofv3 --kernel-trace run, cut from k_ns_zero_band (the band of S0 is cleared) to k_ns_gi (the last launch of the re-projection).  For a
launch that is not on the stream of the factorisation: the kernels of that stream that run while it runs.  Then the figures of the overlap:
the k_chol_panel_band launches with and without a launch of another stream beside them, the tail after the last panel launch, the span.
usage: setup_streams.py <prefix>_kernel_trace.csv [which set-up, counted from the first]"""
import csv, sys
rd = list(csv.DictReader(open(sys.argv[1])))
key = "Stream_Id" if "Stream_Id" in rd[0] else "Queue_Id"
rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", ""), r[key]) for r in rd)
starts = [i for i, r in enumerate(rows) if r[2].startswith("k_ns_zero_band")]
w = int(sys.argv[2]) if len(sys.argv) > 2 else len(starts) // 2
i0 = starts[w]
i1 = next(i for i in range(i0, len(rows)) if rows[i][2].startswith("k_ns_gi"))
seg = rows[i0:i1 + 1]
main = seg[0][3]
on_main = [r for r in seg if r[3] == main]
panels = [r for r in seg if r[2].startswith("k_chol_panel_band")]
other = [r for r in seg if r[3] != main]
t0 = seg[0][0]
print("# one set-up (occurrence %d of k_ns_zero_band; %s of a launch in the last column, %s = the handle's stream):" % (w, key, main))
print("# %d launches, %d on the handle's stream, %.1f us from the first launch to the end of k_ns_gi, %.1f us of kernels" %
      (len(seg), len(on_main), (max(e for _, e, _, _ in seg) - t0) / 1e3, sum(e - s for s, e, _, _ in seg) / 1e3))
alone = [e - s for s, e, _, _ in panels if not any(o[0] < e and o[1] > s for o in other)]
shared = [e - s for s, e, _, _ in panels if any(o[0] < e and o[1] > s for o in other)]
avg = lambda v: "%.1f" % (sum(v) / len(v) / 1e3) if v else "-"
print("# k_chol_panel_band: %d launches, %.1f us from the first to the end of the last; alone %d x %s us, with another stream's launches beside %d x %s us" %
      (len(panels), (panels[-1][1] - panels[0][0]) / 1e3, len(alone), avg(alone), len(shared), avg(shared)))
side_end = max([e for _, e, _, _ in other], default=panels[-1][1])
print("# after the last panel launch: the other streams' launches end %.1f us later; next launch of the handle's stream that is not the count: %.1f us later" %
      ((side_end - panels[-1][1]) / 1e3, (next(r[0] for r in on_main if r[0] >= panels[-1][1] and not r[2].startswith(("k_ns_count_big", "__amd"))) - panels[-1][1]) / 1e3))
print("# %-44s %8s %9s %7s  %s" % ("kernel", "dur_us", "start_us", key[:6], "runs beside (handle's stream)"))
for s, e, n, q in seg:
    beside = "" if q == main else ", ".join(sorted({m[2][:24] for m in on_main if m[0] < e and m[1] > s})) or "-"
    print("# %-44s %8.1f %9.1f %7s  %s" % (n[:44], (e - s) / 1e3, (s - t0) / 1e3, q, beside))
