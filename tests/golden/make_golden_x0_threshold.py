#!/usr/bin/env python3
"""Capture the x0-threshold fixture from the REFERENCE itself (build container only).

Imports the reference's own ``DPM_Solver.dynamic_thresholding_fn`` (deps/dpm_solver_pytorch.py:416-425) and calls it, on the CPU, on fp64
inputs; writes ``x0_threshold.npz`` next to this file.  The reference never travels: the tests only see the fixture.  Usage::

    python tests/golden/make_golden_x0_threshold.py /path/to/reference

(the path may also come from the environment variable NATINF_REFERENCE).

The fixture, for every image size n in SIZES: ``x_<n>`` fp64 [6, n], the rows of ROWS, and for every (ratio, max_val) of ``cases_<n>`` (fp64
[K, 2]) the reference's output ``y_<n>`` fp64 [K, 6, n].  The inputs are multiples of 2^-10 (they compress; the arithmetic does not care).
"""
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
SIZES = (3072, 4, 8, 260)
ROWS = ("ties", "zeros", "nan", "inf", "below", "above")      # quantile below / above max_val = 1 at ratio 0.995
RATIOS, MAX_VALS = (0.995, 0.5, 0.0, 1.0), (1.0, 0.5)


def cases_for(n):
    """every ratio with every max_val for the small sizes; for 3,072 elements the four ratios at max_val 1 and the two middle ones at 0.5"""
    if n == 3072:
        return [(r, 1.0) for r in RATIOS] + [(0.995, 0.5), (0.5, 0.5)]
    return [(r, m) for r in RATIOS for m in MAX_VALS]


def rows_for(n, seed):
    rs = np.random.RandomState(seed)
    grid = lambda scale: np.round(rs.randn(n) * scale * 1024.0) / 1024.0
    x = np.zeros((len(ROWS), n), dtype=np.float64)
    x[0] = rs.randint(-6, 7, size=n) / 4.0                     # thirteen values: every order statistic is a tie
    x[2] = grid(1.0)
    x[2, rs.randint(n)] = np.nan
    x[3] = grid(1.0)
    x[3, 0], x[3, n - 1] = np.inf, -np.inf
    x[4] = grid(0.25)                                          # |x| stays under 1: max_val decides
    x[5] = grid(2.0)                                           # the 0.995 quantile is far above 1
    return x


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("NATINF_REFERENCE", ""))
    src = ref / "deps" / "dpm_solver_pytorch.py"
    if not src.is_file():
        sys.exit(f"usage: {sys.argv[0]} /path/to/reference   ({src} not found)")
    spec = importlib.util.spec_from_file_location("dpm_solver_pytorch", src)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for n in SIZES:
        x = rows_for(n, 1000 + n)
        cases = cases_for(n)
        ys = []
        for ratio, max_val in cases:
            solver = mod.DPM_Solver(None, None, correcting_x0_fn="dynamic_thresholding", thresholding_max_val=max_val,
                                    dynamic_thresholding_ratio=ratio)
            y = solver.dynamic_thresholding_fn(torch.from_numpy(x.copy()), None)
            assert y.dtype == torch.float64 and tuple(y.shape) == x.shape
            ys.append(y.numpy())
        out[f"x_{n}"], out[f"cases_{n}"], out[f"y_{n}"] = x, np.array(cases, dtype=np.float64), np.stack(ys)
    path = HERE / "x0_threshold.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
