#!/usr/bin/env python3
"""Kernel durations of a traced tools/rx_line_times.py run, in dispatch order.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- \\
        python tools/rx_line_times.py --channels C --steps 5 --warmup 2
    python tools/rx_line_ktrace.py DIR C

Prints, per kernel, the last 16 durations in ms.  For k_rx_line the last
steps + warmup are the timed launches (every channel locked), the ones before
them the sync launches; for k_demodulate the first steps + warmup write their
status rows, the next steps + warmup do not, the last one does; k_decode
lists the launches above 1 ms (the others ran under an empty mask).
profiles/rx_line_kernel_trace.txt holds the output for 65,536 and 262,144
channels.
"""
import csv
import glob
import sys

KERNELS = ("k_rx_line_zero", "k_rx_line_mask", "k_rx_line(", "k_demodulate", "k_decode", "k_bin_count", "k_link_rx")


def dur_ms(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6


def main():
    d, label = sys.argv[1], sys.argv[2]
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for name in KERNELS:
        if name == "k_rx_line(":      # the loop kernel itself, however its signature is spelt
            v = [dur_ms(r) for r in rows if "k_rx_line" in r["Kernel_Name"]
                 and "zero" not in r["Kernel_Name"] and "mask" not in r["Kernel_Name"]]
        else:
            v = [dur_ms(r) for r in rows if name in r["Kernel_Name"]]
        if name == "k_decode":
            v = [x for x in v if x > 1.0]
        print(label, name, "n", len(v), "last", " ".join("%.3f" % x for x in v[-16:]))


if __name__ == "__main__":
    main()
