#!/usr/bin/env python3
"""Wall time of the mesh impulse response generator (wv_compressed_waveguide_run) by table length, after a warm-up, and node
updates per second over the work the light cone leaves (sum over steps of tetrahedron(r_k + 1) nodes).  One JSON line per
length; `--check-prefix N` also holds the longest table's first N entries to a table of N taps made separately.

    python tools/compensation_signal_bench.py [--taps 512 2048 4096] [--repeat 3] [--check-prefix 2048]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wayverb_amd import transparent as T  # noqa: E402


def tetrahedron(i):
    return i * (i + 1) * (i + 2) // 6


def node_updates(taps):
    """What the kernel is launched over: step k of 2 dim updates shells 0 .. min(k + 1, 2 dim - 1 - k, dim - 1)."""
    dim = (taps + 1) // 2
    return sum(tetrahedron(min(k + 1, 2 * dim - 1 - k, dim - 1) + 1) for k in range(2 * dim))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taps", type=int, nargs="+", default=[512, 2048, 4096])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--check-prefix", type=int, default=0)
    args = ap.parse_args()
    T.mesh_impulse_response(64)   # code object load, first allocations
    tables = {}
    for taps in args.taps:
        T.mesh_impulse_response(taps)  # warm-up of this size
        times = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            tables[taps] = T.mesh_impulse_response(taps)
            times.append(time.perf_counter() - t0)
        dim = (taps + 1) // 2
        updates = node_updates(taps)
        print(json.dumps(dict(taps=taps, seconds_min=min(times), seconds_all=times, node_updates=updates,
                              whole_wedge_updates=2 * dim * tetrahedron(dim), field_bytes=4 * tetrahedron(dim + 1),
                              updates_per_s=updates / min(times), gb_per_s_at_12B=12 * updates / min(times) / 1e9)), flush=True)
    if args.check_prefix:
        n = args.check_prefix
        short = T.mesh_impulse_response(n)
        longest = tables[max(tables)]
        ok = longest[:n].tobytes() == short.tobytes()
        print(json.dumps(dict(prefix_check=n, against=max(tables), identical=ok)), flush=True)
        if not ok:
            sys.exit(1)


if __name__ == "__main__":
    main()
