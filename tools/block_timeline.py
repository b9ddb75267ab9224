#!/usr/bin/env python3
"""Per-block timeline of the launches around the arma NUTS launch, from a rocprofv3 kernel trace.

    python tools/block_timeline.py <kernel_trace.csv> [last_n_blocks]

For each of the last n (default 5: bench.py's timed repeats) launches of nuts3_kernel: every dispatch from the end of
the PREVIOUS nuts3 launch up to this one's start ("in front") and from its end up to the next nuts3_prep_kernel or the
end of the trace ("behind"), with device durations, their sum and the span they cover (gaps included).  Device-to-device
copies and fills appear as __amd_rocclr_copyBuffer / __amd_rocclr_fillBufferAligned."""
import csv
import sys


def short(name):
    name = name.replace("void ", "").replace("smcn::", "")
    return name.split("(")[0]


def main():
    path = sys.argv[1]
    last_n = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    nuts = [i for i, r in enumerate(rows) if r[2].startswith("nuts3_kernel")]
    sums = {"in front": [], "behind": []}
    for j in nuts[-last_n:]:
        s0, e0, _ = rows[j]
        behind = []
        for r in rows[j + 1:]:
            if r[2].startswith("nuts3_prep_kernel") or r[2].startswith("nuts3_kernel") or r[0] - e0 > 250_000:
                break       # (250 us: what comes later belongs to whatever the driver does after the block)
            behind.append(r)
        # in front: the prep kernel and the fill (cleared counters) next to it
        front = [r for r in rows[max(j - 3, 0):j] if r[2].startswith(("nuts3_prep_kernel", "__amd_rocclr_fill"))]
        print(f"nuts3_kernel {(e0 - s0) / 1e3:9.1f} us")
        for label, part in (("in front", front), ("behind", behind)):
            if not part:
                continue
            total = sum(e - s for s, e, _ in part) / 1e3
            span = ((part[-1][1] - e0) if label == "behind" else (s0 - part[0][0])) / 1e3
            sums[label].append((total, span, len(part)))
            print(f"  {label}: {len(part)} launches, {total:.1f} us of device time, {span:.1f} us from "
                  f"{'the NUTS launch end to the last end' if label == 'behind' else 'the first start to the NUTS launch start'}")
            for s, e, n in part:
                print(f"    {n:48s} {(e - s) / 1e3:7.1f} us   starts {((s - e0) if label == 'behind' else (s - s0)) / 1e3:+9.1f} us")
    for label, v in sums.items():
        if v:
            print(f"mean {label}: {sum(t for t, _, _ in v) / len(v):.1f} us device time, "
                  f"{sum(s for _, s, _ in v) / len(v):.1f} us span, {v[-1][2]} launches")


if __name__ == "__main__":
    main()
