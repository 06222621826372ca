"""The split engine's iterations in a rocprofv3 --kernel-trace CSV: per kernel
the launches and mean duration; over the span from the first cw2_ab to the
last cw2_merge the GPU-busy time (union of kernel intervals), the idle share,
the share of the span in which two kernels run at once, and how much of the
control kernels' time (cw2_ctrl, cw2_merge) lies under a cw2_ab or cw2_az
(zero on one stream; the pipelined decode puts one half's under the other's).

usage: python tools/cw2_overlap.py run_kernel_trace.csv"""
import collections
import csv
import sys


def main(path):
    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("sg::", "").split("<")[0]
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    i0 = next(i for i, r in enumerate(rows) if r[2] == "cw2_ab")
    i1 = max(i for i, r in enumerate(rows) if r[2] == "cw2_merge")
    rows = rows[i0:i1 + 1]
    dur = collections.defaultdict(list)
    for s, e, n in rows:
        dur[n].append(e - s)
    for n, d in sorted(dur.items(), key=lambda x: -sum(x[1])):
        print(f"{n:32s} {len(d):6d} launches  mean {sum(d) / len(d) / 1e3:9.2f} us  total {sum(d) / 1e6:9.3f} ms")
    # sweep: time at depth 0 (idle), >= 2 (overlap); control time under a big kernel
    ev = []
    for s, e, n in rows:
        big = n in ("cw2_ab", "cw2_az")
        small = n in ("cw2_ctrl", "cw2_merge")
        ev.append((s, 1, big, small))
        ev.append((e, -1, big, small))
    ev.sort()
    depth = nbig = nsmall = 0
    idle = over = under = small_t = 0
    last = ev[0][0]
    for t, d, big, small in ev:
        dt = t - last
        if depth == 0:
            idle += dt
        if depth >= 2:
            over += dt
        if nsmall:
            small_t += dt
            if nbig:
                under += dt
        depth += d
        nbig += d * big
        nsmall += d * small
        last = t
    span = rows[-1][1] - rows[0][0]
    it = len(dur["cw2_az"])
    print(f"span {span / 1e6:.3f} ms over {it} cw2_az launches  idle {idle / 1e6:.3f} ms ({idle / span:.2%})  "
          f"two or more kernels at once {over / 1e6:.3f} ms ({over / span:.2%})")
    print(f"control kernels (cw2_ctrl, cw2_merge) run {small_t / 1e6:.3f} ms ({small_t / span:.2%} of the span), "
          f"{under / 1e6:.3f} ms of it under a cw2_ab or cw2_az ({under / max(small_t, 1):.1%})")


if __name__ == "__main__":
    main(sys.argv[1])
