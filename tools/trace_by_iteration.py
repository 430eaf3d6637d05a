#!/usr/bin/env python3
"""Per-iteration view of one kernel in a rocprofv3 kernel trace (rocpd SQLite) of bench.py: the
launches matching a substring, per grid size, in start order; position mod `iters` is the EM
iteration (clean for a grid size only one stream sub-batch has).  Also the share of launches
shorter than 6 us (workgroups that read their trial's flag and return).

  python tools/trace_by_iteration.py <trace dir> backsub4 [iters]
"""
import glob
import os
import sqlite3
import sys

import numpy as np


def main():
    d, pat = sys.argv[1], sys.argv[2]
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    for f in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
        con = sqlite3.connect(f)
        rows = con.execute("select name, grid_x, duration from kernels order by start").fetchall()
        rows = [r for r in rows if pat in r[0]]
        for g in sorted({r[1] for r in rows}):
            du = np.array([r[2] for r in rows if r[1] == g], dtype=float)
            n = len(du) // iters * iters
            if n == 0:
                continue
            mean = du[:n].reshape(-1, iters).mean(axis=0)
            print(f"grid {g}: {len(du)} launches; mean ns by position mod {iters}: "
                  + " ".join(f"{v:.0f}" for v in mean))
        tot = con.execute("select count(*), sum(duration) from kernels").fetchone()
        short = con.execute("select count(*), sum(duration) from kernels where duration < 6000").fetchone()
        print(f"all kernels: {tot[0]} launches {tot[1] / 1e6:.1f} ms; under 6 us: {short[0]} launches "
              f"{(short[1] or 0) / 1e6:.1f} ms")


if __name__ == "__main__":
    main()
