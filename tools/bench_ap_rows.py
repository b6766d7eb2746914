"""ap_tables against ap_tables_rows (2 and 8 thresholds) on one batch: whole calls on the host clock (each call ends in
the download of its tables and the host's step to ApTables), alternating, median / min / max of the repeats after a warm-up of every shape."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import torch  # noqa: E402
from ap_rows_cases import random_scene  # noqa: E402
from gapro_amd.eval_ap_ps_labels import ap_tables, ap_tables_rows  # noqa: E402

S, N, REPS = 64, 150_000, 15
scenes = [random_scene(1000 + i, N, 40, 60) for i in range(S)]
dev = torch.device("cuda:0")
scenes = [[torch.as_tensor(a).to(dev) for a in sc] for sc in scenes]  # inputs resident: no upload in the window
shapes = {"ap_tables": lambda: ap_tables(scenes, "mean_prob"),
          "rows_T2": lambda: ap_tables_rows(scenes, [0.6, 0.8], "mean_prob"),
          "rows_T8": lambda: ap_tables_rows(scenes, [k / 9.0 for k in range(1, 9)], "mean_prob")}
for f in shapes.values():
    f()
times = {k: [] for k in shapes}
for _ in range(REPS):
    for k, f in shapes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        times[k].append((time.perf_counter() - t0) * 1e3)
out = {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}
out.update(scenes=S, points_per_scene=N, reps=REPS)
print(json.dumps(out))
