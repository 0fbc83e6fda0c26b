# Which stream of which context sits on which hardware queue - from a rocprofv3 --kernel-trace run of bench.py (csv output):
#   * per host thread (= context, in bench.py's steps-in-flight region) and stream: the queue its kernels ran on, how many kernels, the kernel launched most
#   * per queue: the (thread, stream) pairs that share it
# Kernels of streams that share a queue run one after the other, whichever context they belong to.
#   python tools/stream_queue_table.py <rocprof output dir>
import csv, glob, os, sys
from collections import Counter, defaultdict


def short(n):
    return n.replace("void ", "").replace("necat::", "").split("(")[0].split("<")[0][:28]


rows = []
for f in sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True)):
    with open(f) as fh:
        rows += list(csv.DictReader(fh))
if not rows:
    raise SystemExit("no kernel_trace.csv under %s" % sys.argv[1])
have_stream = "Stream_Id" in rows[0]
pairs = defaultdict(lambda: [0, 0, Counter(), Counter()])       # (thread, stream) -> kernels, ns, names, queues
for r in rows:
    key = (r.get("Thread_Id", "?"), r["Stream_Id"] if have_stream else "?")
    p = pairs[key]
    p[0] += 1; p[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"]); p[2][short(r["Kernel_Name"])] += 1; p[3][r["Queue_Id"]] += 1
threads = sorted({k[0] for k in pairs}, key=lambda t: -sum(p[0] for k, p in pairs.items() if k[0] == t))
tname = {t: "T%d" % i for i, t in enumerate(threads)}
print("%d kernels, %d host threads, %d (thread, stream) pairs, %d queues%s" % (
    len(rows), len(threads), len(pairs), len({q for p in pairs.values() for q in p[3]}), "" if have_stream else " (this rocprofv3 writes no Stream_Id: one row per thread)"))
print("| thread | stream | queue(s) | kernels | busy ms | most launched |")
print("|---|---|---|---|---|---|")
for (t, s), p in sorted(pairs.items(), key=lambda kv: (threads.index(kv[0][0]), -kv[1][0])):
    print("| %s | %s | %s | %d | %.2f | %s |" % (tname[t], s, " ".join("%s" % q for q, _ in p[3].most_common()), p[0], p[1] / 1e6, p[2].most_common(1)[0][0]))
by_q = defaultdict(list)
for (t, s), p in pairs.items():
    for q in p[3]:
        by_q[q].append("%s/%s" % (tname[t], s))
print()
print("| queue | streams on it (thread/stream) |")
print("|---|---|")
for q in sorted(by_q, key=lambda x: (len(x), x)):
    print("| %s | %s |" % (q, ", ".join(sorted(by_q[q]))))
