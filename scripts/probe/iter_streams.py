"""One interior-point iteration launch by launch with the stream of every launch (development probe): kernel trace CSV of a
rocprofv3 --kernel-trace run, cut at k_ipm_measures.  For a launch that is not on the stream of the measures: the kernels of that stream
that run while it runs.
usage: iter_streams.py <prefix>_kernel_trace.csv [which occurrence of k_ipm_measures]"""
import csv, sys
rd = list(csv.DictReader(open(sys.argv[1])))
key = "Stream_Id" if "Stream_Id" in rd[0] else "Queue_Id"
rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", ""), r[key]) for r in rd)
mk = [i for i, r in enumerate(rows) if r[2].startswith("k_ipm_measures")]
# default: near the middle of the run, the shortest stretch between two measures that factors the k x k matrix (not an LP's last stretch, which holds the polish)
mid = [c for c in range(len(mk) // 2, min(len(mk) // 2 + 6, len(mk) - 1)) if any(r[2].startswith("k_chol_panel_inv") for r in rows[mk[c]:mk[c + 1]])]
w = int(sys.argv[2]) if len(sys.argv) > 2 else min(mid, key=lambda c: mk[c + 1] - mk[c])
seg = rows[mk[w]:mk[w + 1]]
main = seg[0][3]
on_main = [r for r in seg if r[3] == main]
print("# one iteration (occurrence %d of k_ipm_measures; %s of a launch in the last column, %s = the handle's stream):" % (w, key, main))
print("# %d launches, %d on the handle's stream, %.1f us wall, %.1f us of kernels" % (len(seg), len(on_main), (rows[mk[w + 1]][0] - seg[0][0]) / 1e3, sum(e - s for s, e, _, _ in seg) / 1e3))
print("# %-44s %8s %9s %7s  %s" % ("kernel", "dur_us", "start_us", key[:6], "runs beside (handle's stream)"))
t0 = seg[0][0]
for s, e, n, q in seg:
    beside = "" if q == main else ", ".join(sorted({m[2][:24] for m in on_main if m[0] < e and m[1] > s})) or "-"
    print("# %-44s %8.1f %9.1f %7s  %s" % (n[:44], (e - s) / 1e3, (s - t0) / 1e3, q, beside))
