#!/usr/bin/env python3
"""Forward vs post-processing kernel time of the descriptor export from a rocprofv3 --kernel-trace --stats run of
bench_descriptor.py (tools/prof_descriptor.sh).  Post-processing = the kernels after the forward: flattenDetection,
the NMS kernels, the descriptor sampling and the matcher; everything else is the eval forward.  Prints one JSON line."""
import csv
import json
import sys

POST = ("flatten_detection_kernel", "nms_init_kernel", "nms_tiles_kernel", "nms_points_kernel", "sample_desc_kernel",
        "match_dist_kernel", "match_compact_kernel")


def main(stats_csv, steps):
    fwd = post = 0.0
    per = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            name, tot = row["Name"], float(row["TotalDurationNs"])
            k = next((p for p in POST if p in name), None)
            if k:
                post += tot
                per[k] = per.get(k, 0.0) + tot
            else:
                fwd += tot
    us = lambda ns: round(ns / 1e3 / steps, 1)  # noqa: E731
    print(json.dumps({"forward_us_per_step": us(fwd), "post_us_per_step": us(post),
                      "post_share": round(post / (fwd + post), 4) if fwd + post else None,
                      "post_kernels_us_per_step": {k: us(v) for k, v in sorted(per.items())}, "steps_profiled": steps}))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
